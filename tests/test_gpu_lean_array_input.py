"""The lean kernels on GIVEN rays (array input): their draws go through pvt_log_unit and their
Fresnel branch holds no computed critical-angle arm, and neither may show in a single history.  The small lean LSC with
array input is held to the generic family (PVT_NO_LEAN) and to the CPU referee -- integer tallies equal, moment sums
equal up to the order of the atomic additions -- for bundles around the chunk size of the refill, ray tensors that are
row slices (base addresses 8 mod 16), a nonzero ray offset, and a carried stream that runs both the parking and the
closing entries.  A scene whose threshold table holds a NaN (PVT_NO_COS_THRESHOLD) is refused by the lean proof and
must run the generic family, whose computed arm gives the same answer.

The switches are read at scene creation, so each side runs in a FRESH child process (this file, run as a script, is the
worker), each under its own time limit and started only when the one before it has ended well.  The test process itself
never opens the GPU; it computes the referee's side, once."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
SEED, MAXSTEPS = 12345, 1000
SIZES = (1, 63, 64, 65, 4097)            # one ray; one short of a chunk, a chunk, one more; many chunks and an odd end
SLICE_OFFSETS = (1, 5)                   # rows t[off:off + m]: the arrays start 8 bytes off a 16-byte boundary
RAY_OFFSET = 1000
STREAM = (4097,) * 5                     # depth 3: two parking launches, three closing ones
N_RAYS = sum(STREAM)
CASES = [f"n{n}" for n in SIZES] + [f"slice{off}" for off in SLICE_OFFSETS] + ["offset", "stream"]
PARK, USUAL = "trace_kernel_lean_park", "trace_kernel_lean_w4"


def host_rays():
    from pvtrace_amd.engine.emit import emit_bundle
    from tests import scenes

    return emit_bundle(scenes.lsc_equivalent(), N_RAYS, seed=3)[:3]


def case_input(case, rays):
    """(the three arrays of the case, ray offset)"""
    if case.startswith("n"):
        return tuple(a[:int(case[1:])] for a in rays), 0
    if case.startswith("slice"):
        off = int(case[5:])
        return tuple(a[off:off + SIZES[-1]] for a in rays), 0
    if case == "offset":
        return tuple(a[:SIZES[-1]] for a in rays), RAY_OFFSET
    return rays, 0


def _worker(out_path, cases):
    import torch

    from pvtrace_amd.engine import BundlePipeline, compile_scene, native
    from tests import scenes

    dev = torch.device("cuda", 0)
    compiled = compile_scene(scenes.lsc_equivalent())
    on_gpu = tuple(torch.from_numpy(a).to(dev) for a in host_rays())
    out = {}
    dscene = native.DeviceScene(compiled, device=0)
    try:
        for case in cases:
            part, ray_offset = case_input(case, on_gpu)    # (row slices of the resident tensors: no copy)
            if case == "stream":
                pipe = BundlePipeline(dscene, depth=3, carry=True)
                entries, at = [], 0
                try:
                    for k, m in enumerate(STREAM):
                        pipe.submit(tuple(t[at:at + m] for t in part), m, seed=SEED, ray_offset=at, maxsteps=MAXSTEPS, timed=False,
                                    closing=k >= len(STREAM) - 3, tail=k == len(STREAM) - 1)
                        entries.append(dscene.launch_info().get("entry", ""))   # (the lean family's launches name theirs)
                        at += m
                    got = {k: np.asarray(v).copy() for k, v in pipe.totals_host().items()}
                finally:
                    pipe.close()
                out["stream/entries"] = np.array(entries)
            else:
                if case.startswith("slice"):
                    assert part[2].data_ptr() % 16 == 8 and part[0].data_ptr() % 16 == 8
                tallies = dscene.new_tallies()
                dscene.trace(part, part[2].shape[0], SEED, tallies, ray_offset=ray_offset, maxsteps=MAXSTEPS)
                torch.cuda.synchronize()
                got = tallies.host(0)
            out[f"{case}/variant"] = np.array(dscene.launch_info()["variant"])
            for key, value in got.items():
                out[f"{case}/{key}"] = np.asarray(value)
    finally:
        dscene.close()
    np.savez(out_path, **out)


def _run(tmp, label, cases, switch=None):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for name in ("PVT_NO_LEAN", "PVT_NO_COS_THRESHOLD"):
        env.pop(name, None)
    if switch:
        env[switch] = "1"
    path = str(tmp / f"{label}.npz")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), path, ",".join(cases)], cwd=ROOT, env=env, timeout=600,
                          capture_output=True, text=True)
    assert done.returncode == 0, (label, done.returncode, done.stderr[-2000:])
    return dict(np.load(path))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lean_rays")
    lean = _run(tmp, "lean", CASES)                   # (a fault here fails the fixture: nothing else is started)
    generic = _run(tmp, "generic", CASES, "PVT_NO_LEAN")
    refused = _run(tmp, "refused", [f"n{SIZES[-1]}"], "PVT_NO_COS_THRESHOLD")
    return lean, generic, refused


@pytest.fixture(scope="module")
def referee():
    """The CPU referee's tallies of every case -- computed once, never modified."""
    from oracle import oracle as O
    from pvtrace_amd.engine import compile_scene
    from tests import scenes

    compiled = compile_scene(scenes.lsc_equivalent())
    rays = host_rays()
    out = {}
    for case in CASES:
        (pos, dirs, wl), ray_offset = case_input(case, rays)
        out[case] = O.trace_bundle(compiled, pos, dirs, wl, SEED, MAXSTEPS, 128, 0, 8, 0, ray_offset=ray_offset,
                                   math_mode=O.MATH_PORTABLE)
    return out


def assert_equal_tallies(got, case, want, what):
    for key in INT_KEYS:
        assert np.array_equal(got[f"{case}/{key}"], want[key]), (what, case, key)
    assert np.allclose(got[f"{case}/rec_sums"], want["rec_sums"], rtol=1e-11, atol=0), (what, case)


@pytest.mark.gpu
def test_each_side_ran_the_family_it_should(runs):
    lean, generic, refused = runs
    for case in CASES:
        assert str(lean[f"{case}/variant"]) == "lean" and str(generic[f"{case}/variant"]) == "w4", case
    assert lean["stream/entries"].tolist() == [PARK] * 2 + [USUAL] * 3     # both entries ran
    assert str(refused[f"n{SIZES[-1]}/variant"]) == "w4"                    # the NaN threshold sent the scene to the generic family


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_given_rays_equal_the_generic_family_and_the_referee(runs, referee, case):
    lean, generic, _ = runs
    if case != "n1":
        assert referee[case]["rec_crossings"].sum() > 0
    assert_equal_tallies(lean, case, referee[case], "lean against the referee")
    assert_equal_tallies(lean, case, {k: generic[f"{case}/{k}"] for k in INT_KEYS + ("rec_sums",)}, "lean against generic")


@pytest.mark.gpu
def test_a_scene_refused_for_its_threshold_still_computes_the_same(runs, referee):
    _, _, refused = runs
    case = f"n{SIZES[-1]}"
    assert_equal_tallies(refused, case, referee[case], "computed critical-angle arm against the referee")


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2].split(","))
