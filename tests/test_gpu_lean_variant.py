"""The lean kernel family against the generic one, launch for launch: a scene the library proves plain
runs trace_kernel_lean_w4 unless PVT_NO_LEAN is set when the scene is created.  The variant may only leave out code its
proven facts make unreachable, so every history is the generic variant's bit for bit: integer tallies, step counters
and event rows identical; the moment sums equal up to the order of the atomic additions (the tolerance of
tests/test_gpu_carry.py).

The switch is read at scene creation, so each side runs in a FRESH child process (this file, run as a script, is the
worker), under its own time limit; the second is only started when the first has ended well.  The test process itself
never opens the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
SCENES = ("lsc_equivalent", "bench_slab", "fresnel_box", "touching_boxes")
# (bench_slab's spectra are even only up to rounding -- tests/test_lean_variant.py: test_bench_slab_is_lean -- so it runs the
# family's kernels that search the tables; the other scenes and cfg2 run the ones that do not)
BUNDLES = (50_000, 70_001, 64, 30_000, 1, 120_000, 65_000)   # a carried stream of uneven bundles


def _worker(out_path):
    import functools

    import torch

    from benchmarks.configs import cfg2_lsc
    from pvtrace_amd.engine import BundlePipeline, _kernel, compile_scene, native
    from pvtrace_amd.engine.emit import EmitterTables, emit_bundle
    from tests import scenes

    out = {}
    dev = torch.device("cuda", 0)

    def launch(tag, scene, n, seed, device_emission=False, **kw):
        compiled = compile_scene(scene)
        dscene = native.DeviceScene(compiled, device=0, emitter=EmitterTables(scene) if device_emission else None)
        try:
            tallies = dscene.new_tallies()
            if device_emission:
                dscene.trace(None, n, seed, tallies, emit_seed=seed + 1, **kw)
            else:
                pos, dirs, wl, _ = emit_bundle(scene, n, seed=seed + 1)
                rays = tuple(torch.from_numpy(a).to(dev) for a in (pos, dirs, wl))
                dscene.trace(rays, n, seed, tallies, **kw)
            counters = dscene.counters()
            for key, value in tallies.host(0).items():
                out[f"{tag}/{key}"] = value
            out[f"{tag}/steps"] = np.int64(counters["steps"])
            out[f"{tag}/wave_iterations"] = np.int64(counters["wave_iterations"])
            out[f"{tag}/variant"] = np.array(dscene.launch_info()["variant"])
            if kw.get("carry_out"):   # (finish what was parked: nothing stays behind on the stream)
                dscene.trace(None, 0, 0, tallies)
                torch.cuda.synchronize()
        finally:
            dscene.close()

    builders = {"lsc_equivalent": scenes.lsc_equivalent, "bench_slab": functools.partial(scenes.bench_slab, recorders=True),
                "fresnel_box": scenes.fresnel_box, "touching_boxes": scenes.touching_boxes}
    for name in SCENES:
        launch(name, builders[name](), 100_003, 11)
    launch("cfg2", cfg2_lsc(), 1_000_000, 5, device_emission=True)
    # the same lone launch, parking instead of draining: its waves leave the loop when the rays run out (no drain, no tail)
    launch("lsc_parked", scenes.lsc_equivalent(), 100_003, 11, carry_out=True)

    # histories, every ray recorded
    scene = scenes.lsc_equivalent()
    compiled = compile_scene(scene)
    pos, dirs, wl, _ = emit_bundle(scene, 4096, seed=3)
    for key, value in _kernel.trace_bundle(compiled, pos, dirs, wl, 7, 1000, 64, 0, 1, 1).items():
        out[f"history/{key}"] = value
    slab = scenes.bench_slab(recorders=True)   # (the history kernel of the kind that searches its tables)
    spos, sdirs, swl, _ = emit_bundle(slab, 4096, seed=3)
    for key, value in _kernel.trace_bundle(compile_scene(slab), spos, sdirs, swl, 7, 1000, 64, 0, 1, 1).items():
        out[f"history_slab/{key}"] = value

    # a carried stream, three bundles in flight
    dscene = native.DeviceScene(compiled, device=0, emitter=EmitterTables(scene))
    try:
        pipe = BundlePipeline(dscene, depth=3, carry=True)
        at = 0
        for k, m in enumerate(BUNDLES):
            pipe.submit(None, m, seed=5, ray_offset=at, emit_seed=6, tail=(k == len(BUNDLES) - 1))
            at += m
        for key, value in pipe.totals_host().items():
            out[f"stream/{key}"] = np.asarray(value)
        out["stream/variant"] = np.array(dscene.launch_info()["variant"])
    finally:
        dscene.close()
    np.savez(out_path, **out)


def _run(tmp_path, label, no_lean):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("PVT_NO_LEAN", None)
    if no_lean:
        env["PVT_NO_LEAN"] = "1"
    path = str(tmp_path / f"{label}.npz")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=env, timeout=900,
                          capture_output=True, text=True)
    assert done.returncode == 0, (label, done.returncode, done.stderr[-2000:])
    return dict(np.load(path))


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lean")
    lean = _run(tmp, "lean", no_lean=False)       # (a fault here fails the fixture: the generic side is not started)
    generic = _run(tmp, "generic", no_lean=True)
    return lean, generic


@pytest.mark.gpu
def test_the_switch_chooses_the_family(both):
    lean, generic = both
    for tag in SCENES + ("cfg2", "lsc_parked", "stream"):
        assert str(lean[f"{tag}/variant"]) == "lean", tag
        assert str(generic[f"{tag}/variant"]) == "w4", tag


@pytest.mark.gpu
@pytest.mark.parametrize("tag", SCENES + ("cfg2",))
def test_tallies_and_step_counters_equal_the_generic_variants(both, tag):
    lean, generic = both
    for key in INT_KEYS:
        assert np.array_equal(lean[f"{tag}/{key}"], generic[f"{tag}/{key}"]), (tag, key)
    assert np.allclose(lean[f"{tag}/rec_sums"], generic[f"{tag}/rec_sums"], rtol=1e-11), tag
    assert int(lean[f"{tag}/steps"]) == int(generic[f"{tag}/steps"]) > 0, tag     # lane_steps + fused_exits


@pytest.mark.gpu
def test_every_history_row_equals_the_generic_variants(both):
    lean, generic = both
    keys = sorted(k for k in lean if k.startswith(("history/", "history_slab/")))
    assert len(keys) > 16 and int(lean["history/counts"].sum()) > 4096 and int(lean["history_slab/counts"].sum()) > 4096
    for key in keys:
        if key.endswith("/rec_sums"):
            assert np.allclose(lean[key], generic[key], rtol=1e-11)
        else:
            assert np.array_equal(lean[key], generic[key]), key


@pytest.mark.gpu
def test_a_carried_stream_totals_the_same(both):
    lean, generic = both
    for key in INT_KEYS:
        assert np.array_equal(lean[f"stream/{key}"], generic[f"stream/{key}"]), key
    assert np.allclose(lean["stream/rec_sums"], generic["stream/rec_sums"], rtol=1e-11)
    assert int(lean["stream/rec_crossings"].sum()) > sum(BUNDLES)


@pytest.mark.gpu
def test_the_lean_tail_function_runs(both):
    """A lone launch that drains hands its last photons to tail_run<..., LEAN>; the same launch told to park them leaves
    the loop when its rays run out -- the bulk loop alone.  The difference in wave iterations is the drain and the tail
    (which wave claims which rays is a race, so the counts themselves differ from run to run; the steps do not)."""
    lean, generic = both
    assert int(lean["lsc_equivalent/wave_iterations"]) > int(lean["lsc_parked/wave_iterations"]) > 0
    assert int(lean["lsc_parked/steps"]) < int(lean["lsc_equivalent/steps"])


if __name__ == "__main__":
    _worker(sys.argv[1])
