"""The lean kernels' step, one divergent region per lane class, against the generic kernels and the
oracle, at the smallest shapes that reach every boundary of those regions.

The lean variants may regroup the step's divergent bodies but not its arithmetic, its operation order or its draws, so
every history is the generic variant's and the oracle's bit for bit: integer tallies and every event row identical, the
moment sums equal up to the order of the atomic additions (rtol 1e-11, the tolerance of tests/test_gpu_carry.py).
Share of rays that may be skipped or may differ: none.

  * sizes 63, 64, 65 and 4 097: a lane short of a wave, a wave, one lane over, one ray over a round of 64-ray chunks;
  * one launch of each, as a tally launch and with every ray's history recorded, and three carried launches of 200
    photons on one stream;
  * the three emission methods;
  * a slab of two components -- a dye (quantum yield 0.7, both lifetimes) and a one-point background absorber -- so that
    both sides of the component pick, the radiative and the non-radiative end and the lifetime draw all occur, and
    wavelengths below, inside and above the dye's absorption table;
  * a glass cube lit from inside at the critical angle +- 10^-6 ... 1 rad: total internal reflection, partial reflection,
    refraction and the grazing departure that the fused exit must leave to the next step, all in one wave.

The lean / generic switch is read when a scene is created, so each side runs in a FRESH child process (this file, run as
a script, is the worker) under its own time limit; the second is only started when the first has ended well.  The test
process itself never opens the GPU: it runs the oracle (portable math), once per case."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ("rec_distinct", "rec_crossings", "rec_bins")
SIZES = (63, 64, 65, 4097)
METHODS = (0, 1, 2)          # PVT_EMIT_KT, PVT_EMIT_REDSHIFT, PVT_EMIT_FULL
MAX_EVENTS = 48
CARRIED = (200, 200, 200)    # three launches on one stream, the first two parking what they have not finished


def two_component_slab():
    from pvtrace_amd import Absorber, Box, Light, Luminophore, Material, Node, Scene, Sphere, cone
    from pvtrace_amd.data import lumogen_f_red_305
    from tests.scenes import face_recorders

    x = np.arange(400, 800)   # (an even grid bit for bit: the kernels that do not search their tables)
    world = Node(name="world", geometry=Sphere(radius=10.0, material=Material(refractive_index=1.0)))
    Node(name="slab", parent=world, recorders=face_recorders(),
         geometry=Box((2.0, 2.0, 0.5), material=Material(refractive_index=1.5, components=[
             Luminophore(coefficient=np.column_stack((x, lumogen_f_red_305.absorption(x) * 10.0)),
                         emission=np.column_stack((x, lumogen_f_red_305.emission(x))),
                         quantum_yield=0.7, tau_rad=5.0e-9, tau_nr=2.0e-9, name="dye"),
             Absorber(0.4, name="background"),
         ])))
    light = Node(name="light", parent=world, light=Light(direction=functools.partial(cone, np.radians(20)), name="light"))
    light.location = (0.0, 0.0, 3.0)
    light.rotate(np.radians(180), (1, 0, 0))
    return Scene(world)


def slab_rays(scene, n):
    """The light's rays, their wavelengths spread over 380 ... 820 nm: below, inside and above the absorption table."""
    from pvtrace_amd.engine.emit import emit_bundle

    pos, dirs, _, _ = emit_bundle(scene, n, seed=21)
    return pos, dirs, np.linspace(380.0, 820.0, n)


def glass_cube():
    """tests.scenes.fresnel_box -- a cube of n = 1.5 at z = 2 in a spherical world -- with a recorder on every face."""
    from tests.scenes import face_recorders, fresnel_box

    scene = fresnel_box()
    box = [n for n in scene.root.children if n.name == "box"][0]
    box.recorders = face_recorders(hist=False)
    return scene


def critical_angle_rays(n):
    """From the centre of the cube of `glass_cube` (n = 1.5, at z = 2) towards its top face, at the critical
    angle asin(1 / 1.5) +- 10^-6 ... 1 rad: 32 offsets of either sign, repeated to n rays (later copies draw differently)."""
    off = np.logspace(-6.0, 0.0, 32)
    theta = np.arcsin(1.0 / 1.5) + np.concatenate((off, -off))
    theta = np.clip(theta, 1e-3, np.pi / 2 - 1e-3)
    theta = np.resize(theta, n)
    phi = 0.37 * np.arange(n)   # (copies leave through different faces)
    dirs = np.column_stack((np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)))
    pos = np.tile(np.array([0.0, 0.0, 2.0]), (n, 1))
    return pos, dirs, np.full(n, 555.0)


def cases():
    """tag -> (scene builder, rays, seed, emit method, maxsteps); every case runs as a tally launch and as a history launch."""
    out = {}
    for n in SIZES:
        for method in METHODS:
            out[f"slab-{n}-m{method}"] = (two_component_slab, slab_rays, n, 7 + n, method, 300)
    for n in (64, 4097):
        out[f"critical-{n}"] = (glass_cube, lambda scene, n: critical_angle_rays(n), n, 3, 0, 120)
    return out


CASE_TAGS = tuple(f"slab-{n}-m{m}" for n in SIZES for m in METHODS) + ("critical-64", "critical-4097")


def _worker(out_path):
    import torch

    from pvtrace_amd.engine import compile_scene, native

    out = {}
    dev = torch.device("cuda", 0)
    for tag, (build, make_rays, n, seed, method, maxsteps) in cases().items():
        scene = build()
        compiled = compile_scene(scene)
        pos, dirs, wl = make_rays(scene, n)
        rays = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in (pos, dirs, wl))
        dscene = native.DeviceScene(compiled, device=0)
        try:
            tallies = dscene.new_tallies()
            dscene.trace(rays, n, seed, tallies, maxsteps=maxsteps, emit_method=method)
            torch.cuda.synchronize()
            out[f"{tag}/tally/variant"] = np.array(dscene.launch_info()["variant"])
            for key, value in tallies.host(0).items():
                out[f"{tag}/tally/{key}"] = value
            tallies = dscene.new_tallies()
            log = dscene.new_event_columns(n, 1, MAX_EVENTS)
            dscene.trace(rays, n, seed, tallies, log=log, record_every=1, maxsteps=maxsteps, max_events=MAX_EVENTS,
                         emit_method=method)
            torch.cuda.synchronize()
            out[f"{tag}/history/variant"] = np.array(dscene.launch_info()["variant"])
            for key, value in tallies.host(0).items():
                out[f"{tag}/history/{key}"] = value
            for key, value in log.items():
                out[f"{tag}/history/{key}"] = value.cpu().numpy()
        finally:
            dscene.close()

    # three carried launches on one stream: the first two park what is alive when their rays run out
    scene = two_component_slab()
    compiled = compile_scene(scene)
    n = sum(CARRIED)
    pos, dirs, wl = slab_rays(scene, n)
    rays = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev) for a in (pos, dirs, wl))
    dscene = native.DeviceScene(compiled, device=0)
    try:
        tallies = dscene.new_tallies()
        at = 0
        for k, m in enumerate(CARRIED):
            dscene.trace(tuple(t[at:at + m] for t in rays), m, 19, tallies, ray_offset=at, maxsteps=300,
                         carry_out=k < len(CARRIED) - 1)
            at += m
        torch.cuda.synchronize()
        assert not dscene.carry_pending()
        out["carried/tally/variant"] = np.array(dscene.launch_info()["variant"])
        for key, value in tallies.host(0).items():
            out[f"carried/tally/{key}"] = value
    finally:
        dscene.close()
    np.savez(out_path, **out)


def _run(tmp_path, label, no_lean):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("PVT_NO_LEAN", None)
    if no_lean:
        env["PVT_NO_LEAN"] = "1"
    path = str(tmp_path / f"{label}.npz")
    done = subprocess.run([sys.executable, os.path.abspath(__file__), path], cwd=ROOT, env=env, timeout=300,
                          capture_output=True, text=True)
    assert done.returncode == 0, (label, done.returncode, done.stderr[-2000:])
    return dict(np.load(path))


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lean_regions")
    lean = _run(tmp, "lean", no_lean=False)       # (a fault here fails the fixture: the generic side is not started)
    generic = _run(tmp, "generic", no_lean=True)
    return lean, generic


@functools.lru_cache(maxsize=None)
def _oracle(tag, record_every):
    from oracle import oracle as O
    from pvtrace_amd.engine import compile_scene

    if tag == "carried":
        scene = two_component_slab()
        pos, dirs, wl = slab_rays(scene, sum(CARRIED))
        seed, method, maxsteps = 19, 0, 300
    else:
        build, make_rays, n, seed, method, maxsteps = cases()[tag]
        scene = build()
        pos, dirs, wl = make_rays(scene, n)
    return O.trace_bundle(compile_scene(scene), pos, dirs, wl, seed, maxsteps, MAX_EVENTS, method, 4, record_every,
                          math_mode=O.MATH_PORTABLE)


def _same_tallies(got, want, where):
    for key in INT_KEYS:
        assert np.array_equal(np.ravel(got[key]), np.ravel(want[key])), (where, key)
    assert np.allclose(np.ravel(got["rec_sums"]), np.ravel(want["rec_sums"]), rtol=1e-11, atol=0), where


def _side(data, prefix):
    return {k[len(prefix):]: v for k, v in data.items() if k.startswith(prefix)}


@pytest.mark.gpu
def test_the_lean_family_ran(both):
    lean, generic = both
    for tag in CASE_TAGS:
        for mode in ("tally", "history"):
            assert str(lean[f"{tag}/{mode}/variant"]) == "lean", (tag, mode)
            assert str(generic[f"{tag}/{mode}/variant"]) == "w4", (tag, mode)
    assert str(lean["carried/tally/variant"]) == "lean" and str(generic["carried/tally/variant"]) == "w4"


@pytest.mark.gpu
@pytest.mark.parametrize("tag", CASE_TAGS + ("carried",))
def test_tallies_equal_the_generic_kernels_and_the_oracles(both, tag):
    lean, generic = both
    got, ref = _side(lean, f"{tag}/tally/"), _side(generic, f"{tag}/tally/")
    assert int(got["rec_crossings"].sum()) > 0, tag
    _same_tallies(got, ref, (tag, "generic"))
    _same_tallies(got, _oracle(tag, 0), (tag, "oracle"))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", CASE_TAGS)
def test_every_event_row_equals_the_generic_kernels_and_the_oracles(both, tag):
    lean, generic = both
    got, ref, cpu = _side(lean, f"{tag}/history/"), _side(generic, f"{tag}/history/"), _oracle(tag, 1)
    _same_tallies(got, ref, (tag, "generic"))
    _same_tallies(got, cpu, (tag, "oracle"))
    n = cases()[tag][2]
    assert got["counts"].shape[0] == n and int(got["counts"].sum()) > n, tag
    columns = sorted(k for k in got if k not in INT_KEYS + ("rec_sums", "variant"))
    assert len(columns) > 10
    for key in columns:
        assert np.array_equal(np.ravel(got[key]), np.ravel(ref[key])), (tag, "generic", key)
        assert np.array_equal(np.ravel(got[key]), np.ravel(cpu[key])), (tag, "oracle", key)


EV_REFLECT, EV_TRANSMIT, EV_ABSORB, EV_NONRADIATIVE, EV_EMIT, EV_EXIT, EV_KILL = 1, 2, 3, 4, 6, 7, 9   # include/pvtrace_hip.h


def _rows(log):
    """(kind, component, duration) of the rows that were written, and the kind of every ray's first event."""
    at = np.concatenate([np.arange(c) + j * MAX_EVENTS for j, c in enumerate(log["counts"])])
    first = np.ravel(log["kind"])[np.arange(len(log["counts"])) * MAX_EVENTS + 1]   # (row 0 is GENERATE)
    return np.ravel(log["kind"])[at], np.ravel(log["component"])[at], np.ravel(log["duration"])[at], first


def test_the_cases_reach_every_region_boundary():
    """What the shapes are chosen for, read from the oracle's event rows (no GPU): in ONE wave of the slab both components
    absorb and the dye's decision ends both ways, with a lifetime drawn; in ONE wave at the cube total internal reflection,
    partial reflection and refraction all occur, and photons trapped by total reflection run into the step limit."""
    kind, comp, duration, _ = _rows(_oracle("slab-64-m0", 1))
    for k in (EV_ABSORB, EV_EMIT, EV_NONRADIATIVE, EV_REFLECT, EV_TRANSMIT, EV_EXIT):
        assert k in kind, k
    assert len(set(comp[kind == EV_ABSORB])) == 2             # both sides of the component pick
    # (a flight of 3 cm takes 1.5e-10 s: a duration of nanoseconds is a drawn lifetime)
    assert duration[kind == EV_EMIT].max() > 1e-9 and duration[kind == EV_NONRADIATIVE].max() > 1e-9
    kind, _, _, first = _rows(_oracle("critical-64", 1))
    above, below = first[:32], first[32:]                     # the critical angle + offsets, - offsets
    steep = np.logspace(-6.0, 0.0, 32) < 0.05                 # (within 45 degrees of the axis the top face is the one hit)
    assert steep.sum() > 20 and (above[steep] == EV_REFLECT).all()   # beyond the critical angle: every one reflected
    assert EV_TRANSMIT in below and EV_REFLECT in below       # inside it: refraction, and partial reflection
    assert EV_KILL in kind or (_oracle("critical-64", 1)["counts"] >= MAX_EVENTS - 1).any()


if __name__ == "__main__":
    _worker(sys.argv[1])
