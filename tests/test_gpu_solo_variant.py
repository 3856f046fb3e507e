"""The solo entries against the lean family's own, launch for launch, and against the CPU referee:
the tally launches of a scene the library proves solo -- one unrotated box in a lazy root, pvt_scene_pack.h: prove_solo --
run trace_kernel_solo_park / trace_kernel_solo_fin unless PVT_NO_SOLO is set when the scene is created.  Their node stage
selects one of three outcomes instead of folding crossings, and a wave with a lane it does not cover (undecided by the
root's bound, a direction component below 1e-300, a slab miss) runs the node loop itself: every history is the lean
kernels' bit for bit.  Integer tallies are compared exactly, the moment sums to the 1e-12 of tests/test_gpu_parity.py.

The switch is read at scene creation, so each side runs in a FRESH child process (this file, run as a script, is the
worker), under its own time limit; the second is only started when the first has ended well.  The test process itself
never opens the GPU; it runs the referee, once per case."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
SIZES = (64, 257, 20_000)        # one wave; a ragged handful; many workgroups, the drain and the tail function
WORLDS = ("box", "sphere")
KINDS = ("inside", "outside_hit", "outside_miss", "on_face", "zero_components", "root_edge", "behind")
# the child's centre: translated off the origin in one world, at it in the other; halves and centres are dyadic, so a
# start "exactly on a face" is exactly there in the kernel's own pos + translation as well
CENTRE = {"box": np.array([0.25, -0.5, 0.5]), "sphere": np.array([0.0, 0.0, 0.0])}
HALF = np.array([1.0, 1.5, 0.5])
SEED, MAXSTEPS = 5, 200
GRAZING = (("box", 1.0), ("sphere", 1.0), ("box", 1.5), ("sphere", 1.05))
GRAZING_N = 100_000
STREAM = (20_000, 64, 257, 5_000, 12_000)   # a carried stream: five launches, three in flight


def slab_scene(world, index=1.5, dye=True):
    """One box of 2 x 3 x 1 in a world that is a box or a sphere; a dye and a background absorber, so that absorption and
    re-emission are on the path too (or nothing at all: the grazing case's clear slab)."""
    from pvtrace_amd import Absorber, Box, Luminophore, Material, Node, Scene, Sphere
    from pvtrace_amd.data import lumogen_f_red_305
    from tests import scenes

    geometry = Box((300.0, 300.0, 300.0), material=Material(refractive_index=1.0)) if world == "box" else \
        Sphere(radius=200.0, material=Material(refractive_index=1.0))
    root = Node(name="world", geometry=geometry)
    x = np.arange(400, 800)
    components = [Luminophore(coefficient=np.column_stack((x, lumogen_f_red_305.absorption(x) * 2.0)),
                              emission=np.column_stack((x, lumogen_f_red_305.emission(x))), quantum_yield=0.95, name="dye"),
                  Absorber(0.05, name="host")] if dye else []
    slab = Node(name="slab", geometry=Box(tuple(2.0 * HALF), material=Material(refractive_index=index, components=components)),
                parent=root, recorders=scenes.face_recorders(hist=dye))
    slab.location = tuple(CENTRE[world])
    return Scene(root)


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def rays_of(world, kind, n):
    """The starting rays of a case (positions, directions, wavelengths): the same in the worker and in the test."""
    rng = np.random.default_rng(1000 * WORLDS.index(world) + 10 * KINDS.index(kind) + SIZES.index(n))
    centre = CENTRE[world]
    d = _unit(rng.normal(size=(n, 3)))
    if kind == "inside":
        local = (rng.random((n, 3)) * 2 - 1) * HALF * 0.999
    elif kind == "outside_hit":        # from a shell around the slab towards a point inside it
        local = _unit(rng.normal(size=(n, 3))) * rng.uniform(3.0, 40.0, (n, 1))
        d = _unit((rng.random((n, 3)) * 2 - 1) * HALF * 0.9 - local)
    elif kind == "outside_miss":       # from the shell outwards, and along the slab's faces past it
        local = _unit(rng.normal(size=(n, 3))) * rng.uniform(3.0, 40.0, (n, 1))
        d = _unit(local + 0.5 * rng.normal(size=(n, 3)))
        half = n // 2
        d[:half] = _unit(np.cross(local[:half], rng.normal(size=(half, 3))))   # (at right angles to the way in: misses by >= 3 - |half|)
    elif kind == "on_face":            # exactly on a face, and within 1e-13 of it on either side; heading in and out
        local = (rng.random((n, 3)) * 2 - 1) * HALF * 0.999
        rows = np.arange(n)
        axis = rng.integers(0, 3, n)
        sign = rng.choice([-1.0, 1.0], n)
        off = np.choose(rows % 5, [0.0, 1e-13, -1e-13, 3e-14, -3e-14])
        local[rows, axis] = sign * (HALF[axis] + off)
    elif kind == "zero_components":    # one and two direction components exactly zero, from inside and from outside
        local = (rng.random((n, 3)) * 2 - 1) * HALF * np.where(np.arange(n)[:, None] % 2 == 0, 0.999, 4.0)
        rows = np.arange(n)
        axis = rng.integers(0, 3, n)
        d[rows, axis] = 0.0
        two = rows % 3 == 0
        d[rows[two], (axis[two] + 1) % 3] = 0.0
        d = _unit(d)
        assert np.all(np.sum(d == 0.0, axis=1) >= 1) and np.any(np.sum(d == 0.0, axis=1) == 2)
    elif kind == "behind":             # outside, heading away along a line through the box: tmin <= tmax <= kEps in every lane,
        inner = (rng.random((n, 3)) * 2 - 1) * HALF * 0.9   # so whole waves take the closed form's third outcome
        local = inner + d * rng.uniform(3.0, 40.0, (n, 1))
    elif kind == "root_edge":          # outside the root, on it, a hair inside it, anywhere inside it; heading inwards
        reach = 200.0 if world == "sphere" else 150.0
        u = _unit(rng.normal(size=(n, 3)))
        scale = np.concatenate([np.full(n // 4, 1.2), np.full(n // 4, 1.0), np.full(n // 4, 1.0 - 1e-13), rng.random(n - 3 * (n // 4))])
        if world == "box":
            u = u / np.max(np.abs(u), axis=1)[:, None]   # (onto the cube's surface)
        d = _unit(-u + 0.01 * rng.normal(size=(n, 3)))   # (towards the slab: within ~1 cm of its centre from 150 cm)
        return u * (reach * scale)[:, None], d, np.full(n, 555.0)
    else:
        raise ValueError(kind)
    wl = np.where(np.arange(n) % 2 == 0, 555.0, 470.0)   # (470 nm: absorbed within the slab more often than not)
    return local + centre, d, wl


def grazing_rays(world, n=GRAZING_N):
    """tests/test_gpu_parity.py: test_fused_exit_clears_grazing_departures_exactly, its rays at another size: a third start
    just inside a face and head out of it at 1e-9..1e-2 rad, a third start just outside and graze it, the rest are random."""
    rng = np.random.default_rng(77)
    centre = np.array([0.3, -0.2, 0.5])
    local = (rng.random((n, 3)) * 2 - 1) * HALF * 0.999
    d = _unit(rng.normal(size=(n, 3)))
    k = 2 * n // 3
    axis = rng.integers(0, 3, k)
    sign = rng.choice([-1.0, 1.0], k)
    gap = 10.0 ** rng.uniform(-12, -3, k)
    slope = 10.0 ** rng.uniform(-9, -2, k)
    inside = np.arange(k) < k // 2
    rows = np.arange(k)
    local[rows, axis] = sign * (HALF[axis] + np.where(inside, -gap, gap))
    d[rows, axis] = np.where(inside, sign, -sign) * slope
    return local + centre, _unit(d), np.full(n, 555.0)


def grazing_scene(world, index):
    from pvtrace_amd import Scene

    scene = slab_scene(world, index=index, dye=False)
    slab = next(iter(scene.root.children))
    slab.location = (0.3, -0.2, 0.5)
    return Scene(scene.root)


def case_tags():
    return tuple(f"{w}/{k}/{n}" for w in WORLDS for k in KINDS for n in SIZES)


GRAZING_RUNS = tuple((f"grazing/{w}-{i}/{m}", w, i, m, stride) for w, i in GRAZING
                     for m, stride in ((1000, 1), (1, 10), (2, 10), (3, 10)))


def _worker(out_path):
    import torch

    from pvtrace_amd.engine import BundlePipeline, compile_scene, native
    from pvtrace_amd.engine.emit import EmitterTables
    from tests import scenes

    out = {}
    dev = torch.device("cuda", 0)

    def on_device(arrays):
        return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in arrays)

    def tally(tag, dscene, rays, n, maxsteps):
        dscene.counters(reset=True)
        tallies = dscene.new_tallies()
        dscene.trace(rays, n, SEED, tallies, maxsteps=maxsteps)
        torch.cuda.synchronize()
        for key, value in tallies.host(0).items():
            out[f"{tag}/{key}"] = value
        out[f"{tag}/solo"] = np.array(dscene.solo())
        out[f"{tag}/steps"] = np.int64(dscene.counters()["steps"])

    for world in WORLDS:
        dscene = native.DeviceScene(compile_scene(slab_scene(world)), device=0)
        try:
            for kind in KINDS:
                for n in SIZES:
                    tally(f"{world}/{kind}/{n}", dscene, on_device(rays_of(world, kind, n)), n, MAXSTEPS)
            # a history launch of the same scene keeps the lean family's own kernel
            n = 257
            rays = on_device(rays_of(world, "inside", n))
            log = dscene.new_event_columns(n, 1, 32)
            dscene.trace(rays, n, SEED, dscene.new_tallies(), log=log, record_every=1, maxsteps=MAXSTEPS, max_events=32)
            torch.cuda.synchronize()
            out[f"{world}/history/solo"] = np.array(dscene.solo())
            out[f"{world}/history/variant"] = np.array(dscene.launch_info()["variant"])
            dscene.trace(rays, n, SEED, dscene.new_tallies(), maxsteps=MAXSTEPS)
            torch.cuda.synchronize()
            out[f"{world}/tally_again/solo"] = np.array(dscene.solo())
            out[f"{world}/tally_again/variant"] = np.array(dscene.launch_info()["variant"])
        finally:
            dscene.close()

    for world, index in GRAZING:
        dscene = native.DeviceScene(compile_scene(grazing_scene(world, index)), device=0)
        try:
            pos, d, wl = grazing_rays(world)
            for tag, w, i, maxsteps, stride in GRAZING_RUNS:
                if (w, i) == (world, index):
                    tally(tag, dscene, on_device((pos[::stride], d[::stride], wl[::stride])), len(pos[::stride]), maxsteps)
        finally:
            dscene.close()

    # a carried stream through the pipeline: park and resume between the solo entries
    scene = scenes.lsc_equivalent()
    dscene = native.DeviceScene(compile_scene(scene), device=0, emitter=EmitterTables(scene))
    try:
        pipe = BundlePipeline(dscene, depth=3, carry=True)
        at, solo, entries = 0, [], []
        for k, m in enumerate(STREAM):
            pipe.submit(None, m, seed=5, ray_offset=at, emit_seed=6, tail=(k == len(STREAM) - 1))
            solo.append(dscene.solo())
            entries.append(dscene.launch_info()["entry"])
            at += m
        for key, value in pipe.totals_host().items():
            out[f"stream/{key}"] = np.asarray(value)
        out["stream/solo"] = np.array(solo)
        out["stream/entries"] = np.array(entries)
        out["stream/variant"] = np.array(dscene.launch_info()["variant"])
    finally:
        dscene.close()
    np.savez(out_path, **out)


def _run(tmp_path, label, no_solo):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("PVT_NO_SOLO", None)
    if no_solo:
        env["PVT_NO_SOLO"] = "1"
    path = str(tmp_path / f"{label}.npz")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=env, timeout=600,
                          capture_output=True, text=True)
    assert done.returncode == 0, (label, done.returncode, done.stderr[-2000:])
    return dict(np.load(path))


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("solo")
    solo = _run(tmp, "solo", no_solo=False)       # (a fault here fails the fixture: the other side is not started)
    lean = _run(tmp, "lean", no_solo=True)
    return solo, lean


@functools.lru_cache(maxsize=None)
def referee(tag):
    """The CPU referee's tallies and loop count for one case: computed once, shared, never changed."""
    from oracle import oracle as O
    from pvtrace_amd.engine import compile_scene

    parts = tag.split("/")
    if parts[0] == "grazing":
        _, world, index, maxsteps, stride = next(r for r in GRAZING_RUNS if r[0] == tag)
        compiled = compile_scene(grazing_scene(world, index))
        pos, d, wl = (a[::stride] for a in grazing_rays(world))
    else:
        world, kind, n = parts[0], parts[1], int(parts[2])
        compiled, maxsteps = compile_scene(slab_scene(world)), MAXSTEPS
        pos, d, wl = rays_of(world, kind, n)
    cpu = O.trace_bundle(compiled, pos, d, wl, SEED, maxsteps, 16, 0, 1, 0, math_mode=O.MATH_PORTABLE)
    return cpu, O.last_steps()


def _same_tallies(got, want, tag, what):
    for key in INT_KEYS:
        assert np.array_equal(np.asarray(got[f"{tag}/{key}"]).ravel(), np.asarray(want[key]).ravel()), (tag, what, key)
    assert np.allclose(np.asarray(got[f"{tag}/rec_sums"]).ravel(), np.asarray(want["rec_sums"]).ravel(), rtol=1e-12, atol=0.0), (tag, what)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", case_tags() + tuple(r[0] for r in GRAZING_RUNS))
def test_solo_tallies_equal_the_lean_kernels_and_the_referees(both, tag):
    solo, lean = both
    assert bool(solo[f"{tag}/solo"]) and not bool(lean[f"{tag}/solo"]), tag
    cpu, _ = referee(tag)
    _same_tallies(solo, cpu, tag, "solo against the referee")
    _same_tallies(lean, cpu, tag, "PVT_NO_SOLO against the referee")
    _same_tallies(solo, {k: lean[f"{tag}/{k}"] for k in INT_KEYS + ("rec_sums",)}, tag, "solo against PVT_NO_SOLO")
    assert int(solo[f"{tag}/steps"]) == int(lean[f"{tag}/steps"]), tag


@pytest.mark.gpu
def test_the_cases_reach_what_they_are_for(both):
    solo, _ = both
    for world in WORLDS:
        for kind in ("inside", "outside_hit", "on_face", "zero_components"):
            assert int(solo[f"{world}/{kind}/20000/rec_crossings"].sum()) > 5_000, (world, kind)
        # (the quarter that starts anywhere inside the root, aimed at the slab, at the least)
        assert int(solo[f"{world}/root_edge/20000/rec_crossings"].sum()) > 1_000, world
        # rays that miss the slab, or leave it behind them, cross nothing
        assert int(solo[f"{world}/outside_miss/20000/rec_crossings"].sum()) == 0, world
        assert int(solo[f"{world}/behind/20000/rec_crossings"].sum()) == 0, world
    for tag, _, _, maxsteps, _ in GRAZING_RUNS:
        if maxsteps == 1000:
            assert int(solo[f"{tag}/rec_crossings"].sum()) > GRAZING_N // 2, tag


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_kernels_own_counters_equal_the_referees_loop_count(both, world, kind):
    solo, _ = both
    tag = f"{world}/{kind}/20000"
    _, loops = referee(tag)
    assert int(solo[f"{tag}/steps"]) == loops > 0, tag     # lane_steps + fused_exits


@pytest.mark.gpu
def test_only_tally_launches_are_solo(both):
    solo, lean = both
    for world in WORLDS:
        assert not bool(solo[f"{world}/history/solo"]) and str(solo[f"{world}/history/variant"]) == "lean", world
        assert bool(solo[f"{world}/tally_again/solo"]) and str(solo[f"{world}/tally_again/variant"]) == "lean", world
        assert not bool(lean[f"{world}/tally_again/solo"]) and str(lean[f"{world}/tally_again/variant"]) == "lean", world


@pytest.mark.gpu
def test_a_carried_stream_totals_the_same(both):
    solo, lean = both
    assert solo["stream/solo"].all() and not lean["stream/solo"].any()
    assert str(solo["stream/variant"]) == str(lean["stream/variant"]) == "lean"
    # the family's entries are reported as before: the parking one for the launches that park
    assert list(solo["stream/entries"]) == list(lean["stream/entries"])
    assert "trace_kernel_lean_park" in list(solo["stream/entries"])
    for key in INT_KEYS:
        assert np.array_equal(solo[f"stream/{key}"], lean[f"stream/{key}"]), key
    assert np.allclose(solo["stream/rec_sums"], lean["stream/rec_sums"], rtol=1e-12, atol=0.0)
    assert int(solo["stream/rec_crossings"].sum()) > sum(STREAM)


if __name__ == "__main__":
    _worker(sys.argv[1])
