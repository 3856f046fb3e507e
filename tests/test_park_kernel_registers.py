"""The parking entries of the lean family (`trace_kernel_lean_park`, trace_body's PARK form), read from the code object
inside libpvtrace_hip.so (no GPU needed).  A launch that parks its survivors can reach neither the drain rendezvous nor
`tail_run`; compiled without them the step loop alone decides the registers, and that is what lets a fifth wave onto a
SIMD: 512 vector registers / 5 waves, in the allocation granule of 8, is 96."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pvtrace_amd", "csrc", "libpvtrace_hip.so")


@pytest.fixture(scope="module")
def kernels():
    import __graft_entry__ as entry

    meta = entry.kernel_metadata(LIB)       # the same reader build() warns with
    if not meta:
        pytest.skip("library or LLVM binutils not present")
    return meta


def _template_args(name, stem):
    """The boolean template arguments in a mangled kernel name, after `stem`: 'ILb0ELb1E...' -> (False, True, ...)."""
    tail = name.split(stem, 1)[1]
    args = []
    while tail.startswith(("ILb", "Lb")):
        tail = tail[tail.index("Lb") + 2:]
        args.append(tail[0] == "1")
        tail = tail[2:]
    return tuple(args)


def test_the_parking_entries_fit_five_waves_per_simd(kernels):
    park = {_template_args(n, "trace_kernel_lean_park"): m for n, m in kernels.items() if "trace_kernel_lean_park" in n}
    lean = {_template_args(n, "trace_kernel_lean_w4"): m for n, m in kernels.items() if "trace_kernel_lean_w4" in n}
    # {rays, emitter} x {searched, even}; the family's usual entries: {tally, history} x the same
    assert sorted(park) == [(False, False), (False, True), (True, False), (True, True)], sorted(park)
    assert len(lean) == 8
    for (emit, even), m in park.items():
        usual = lean[(False, emit, even)]   # the tally launch of the same kind that finishes its own photons
        # the fifth wave: a condition, not a measurement
        assert m["vgpr_count"] <= 96, ((emit, even), m)
        # at most one 64-bit value parked OUTSIDE the loop (the emitter kinds keep one around their calls); the loop
        # itself holds no scratch instruction (read in the ISA: profiles/lean_park.md)
        assert m["vgpr_spill_count"] <= 2, ((emit, even), m)
        # no frame for `tail_run`: never more scratch than the usual entry
        assert m["private_segment_fixed_size"] <= usual["private_segment_fixed_size"], ((emit, even), m, usual)


def test_the_build_time_warning_knows_the_parking_entries(kernels):
    import __graft_entry__ as entry

    assert entry.check_kernel_budgets() == []
    # ... and speaks up when one of them leaves its budget
    broken = {n: dict(m, vgpr_count=104) if "trace_kernel_lean_park" in n else m for n, m in kernels.items()}
    problems = entry.check_kernel_budgets(broken)
    assert len(problems) == 4 and all("trace_kernel_lean_park" in p for p in problems), problems
