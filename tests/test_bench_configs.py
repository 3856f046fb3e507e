"""bench.py's scenes are built with the product API alone (benchmarks/configs.py); they must flatten to the very
tables the parity tests and the golden fixtures use (tests/scenes.py), and the host-side helpers of the bench
must behave without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from benchmarks import configs
from pvtrace_amd.engine import compile_scene
from tests import scenes
from tests.util import assert_same_tables, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_scenes_flatten_to_the_tested_tables():
    for mine, theirs in ((configs.cfg2_lsc, scenes.lsc_equivalent), (configs.cfg4_nested_cylinders, scenes.nested_cylinders),
                         (configs.cfg5_coated_slab, scenes.coated_slab)):
        a, b = compile_scene(mine()), compile_scene(theirs())
        ta, tb = a.tables(), b.tables()
        assert ta.keys() == tb.keys()
        for key in ta:
            assert np.array_equal(np.asarray(ta[key]), np.asarray(tb[key])), (mine.__name__, key)
        assert a.recorder_names == b.recorder_names and a.node_names == b.node_names
    # the headline scene IS the scene of the 10^6-photon reference fixture; cfg4 likewise
    assert_same_tables(compile_scene(configs.cfg2_lsc()), load_golden("tallies_lsc_1e6.npz"))
    assert_same_tables(compile_scene(configs.cfg4_nested_cylinders()), load_golden("tallies_nested_cylinders_1e6.npz"))


def test_rank_pinning_partitions_the_allowed_cores():
    allowed = sorted(os.sched_getaffinity(0))
    try:
        if len(allowed) >= 2:
            world = 2
            slices = []
            for r in range(world):
                os.sched_setaffinity(0, allowed)
                slices.append(bench.pin_rank_to_cores(r, world))
            assert all(s for s in slices) and not set(slices[0]) & set(slices[1])
            assert set(slices[0]) | set(slices[1]) <= set(allowed)
        assert bench.pin_rank_to_cores(0, 1) is None
    finally:
        os.sched_setaffinity(0, allowed)
    assert 1 <= bench.usable_cores() <= len(allowed)


def test_bench_without_a_gpu_fails_loudly_with_an_error_line():
    """No CPU path: on a box without a GPU the bench must say so (and print the line the driver reads)."""
    import torch

    if torch.cuda.is_available():
        return
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    done = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1"], env=env, cwd=ROOT,
                          capture_output=True, text=True, timeout=600)
    assert done.returncode != 0 and "no CPU path" in (done.stdout + done.stderr)


def test_a_plain_bench_run_is_the_headline_alone_and_full_brings_the_other_legs_back(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "2"])
    plain = bench.parse_args()
    assert (plain.steps, plain.warmup, plain.repeats, plain.sustained_s, plain.total_photons) == (7, 2, 0, 0.0, 0)
    assert plain.extra_configs == plain.scene_sizes == "none" and plain.no_cpu_baseline and not plain.full
    assert plain.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    full = bench.parse_args()
    assert (full.repeats, full.sustained_s, full.total_photons) == (15, 12.5, 100_000_000)
    assert full.extra_configs == "cfg4,cfg5" and full.scene_sizes == "1,3,6,11" and not full.no_cpu_baseline
    assert full.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--repeats", "2", "--extra-configs", "none", "--no-cpu-baseline"])
    mixed = bench.parse_args()   # a leg's own flag wins over the default --full gives it
    assert mixed.repeats == 2 and mixed.extra_configs == "none" and mixed.no_cpu_baseline


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_a_plain_bench_run_times_its_steps_and_dumps_the_tallies_of_its_window(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR`: one window of K steps, the line's `ms_per_step` is that
    window's seconds / K, and DIR holds the tallies the timed steps produced -- the same counts the line's fractions
    come from, every photon of the window in `entering` + `reflected`."""
    import json

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    steps, photons = 5, 50_000
    done = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                           "--warmup", "2", "--photons", str(photons), "--ray-buffers", "2",
                           "--dump-outputs", str(tmp_path / "out")], env=env, cwd=ROOT, capture_output=True, text=True,
                          timeout=500)
    assert done.returncode == 0, done.stderr[-2000:]
    out = json.loads([l for l in done.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == steps and out["repeats"]["windows"] == 1 and out["value"] > 0 and "error" not in out
    assert out["unit"] == "photons/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert abs(out["ms_per_step"] * 1e-3 * steps * out["value"] - photons * steps) < 1e-6 * photons * steps
    for leg in ("roofline", "sustained", "strong_scaling", "configs", "scene_scaling", "meshes", "extra", "cpu_baseline"):
        assert leg not in out, leg
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == ["rec_bins.npy", "rec_crossings.npy", "rec_distinct.npy", "rec_sums.npy"], files
    arrays = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert all(a.dtype == np.float64 for a in arrays.values())
    names = list(out["tallies"])
    distinct = arrays["rec_distinct"]
    assert distinct.shape == (len(names),)
    assert np.allclose(distinct / (photons * steps), [out["tallies"][k] for k in names], rtol=0, atol=1e-15)
    assert distinct[names.index("entering")] + distinct[names.index("reflected")] == photons * steps
