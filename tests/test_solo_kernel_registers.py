"""The solo entries (`trace_kernel_solo_park`, `trace_kernel_solo_fin`: trace_body's SOLO form), read from the code object
inside libpvtrace_hip.so (no GPU needed), the way tests/test_kernel_registers.py and tests/test_park_kernel_registers.py
read theirs.  The parking entries keep the fifth wave of the lean family's (96 vector registers, at most one 64-bit value
parked outside the loop, no scalar register spilled, no frame of a tail function); the finishing entries keep four waves
with no vector register spilled and no more scratch than the frame of the function they call."""
import pytest

from tests.test_kernel_registers import CALL_FRAME
from tests.test_park_kernel_registers import LIB, _template_args


@pytest.fixture(scope="module")
def kernels():
    import __graft_entry__ as entry

    meta = entry.kernel_metadata(LIB)
    if not meta:
        pytest.skip("library or LLVM binutils not present")
    return meta


KINDS = [(False, False), (False, True), (True, False), (True, True)]   # {rays, emitter} x {searched, even}


def test_there_are_eight_solo_entries_and_the_old_counts_stand(kernels):
    park = [n for n in kernels if "trace_kernel_solo_park" in n]
    fin = [n for n in kernels if "trace_kernel_solo_fin" in n]
    assert sorted(_template_args(n, "trace_kernel_solo_park") for n in park) == KINDS
    assert sorted(_template_args(n, "trace_kernel_solo_fin") for n in fin) == KINDS
    for n in park + fin:   # (what the older tests count by substring stays what it was)
        assert "trace_kernel_lean_park" not in n and "trace_kernel_lean_w4" not in n and "trace_kernel_w4" not in n, n
    assert len([n for n in kernels if "trace_kernel_lean_park" in n]) == 4
    assert len([n for n in kernels if "trace_kernel_lean_w4" in n]) == 8


def test_the_solo_parking_entries_fit_five_waves_per_simd(kernels):
    park = {_template_args(n, "trace_kernel_solo_park"): m for n, m in kernels.items() if "trace_kernel_solo_park" in n}
    fin = {_template_args(n, "trace_kernel_solo_fin"): m for n, m in kernels.items() if "trace_kernel_solo_fin" in n}
    for kind, m in park.items():
        assert m["vgpr_count"] <= 96, (kind, m)
        assert m["vgpr_spill_count"] <= 2, (kind, m)
        assert m["sgpr_spill_count"] == 0, (kind, m)
        assert m["private_segment_fixed_size"] <= fin[kind]["private_segment_fixed_size"], (kind, m, fin[kind])


def test_the_solo_finishing_entries_fit_four_waves_and_spill_nothing(kernels):
    fin = {_template_args(n, "trace_kernel_solo_fin"): m for n, m in kernels.items() if "trace_kernel_solo_fin" in n}
    for kind, m in fin.items():
        assert m["vgpr_count"] <= 128, (kind, m)
        assert m["vgpr_spill_count"] == 0, (kind, m)
        assert m["private_segment_fixed_size"] <= CALL_FRAME, (kind, m)
        # scalar registers ARE spilled here, as in the lean family's usual entries (to lanes of a vector register, no
        # memory): held to the budget the build-time check keeps for a four-wave kernel's loop
        assert m["sgpr_spill_count"] <= 60, (kind, m)


def test_the_build_time_warning_knows_the_solo_entries(kernels):
    import __graft_entry__ as entry

    assert entry.check_kernel_budgets() == []
    broken = {n: dict(m, vgpr_count=104) if "trace_kernel_solo_park" in n else m for n, m in kernels.items()}
    problems = entry.check_kernel_budgets(broken)
    assert len(problems) == 4 and all("trace_kernel_solo_park" in p for p in problems), problems
    broken = {n: dict(m, vgpr_spill_count=1) if "trace_kernel_solo_fin" in n else m for n, m in kernels.items()}
    problems = entry.check_kernel_budgets(broken)
    assert len(problems) == 4 and all("trace_kernel_solo_fin" in p for p in problems), problems
