"""The launch's choice of kernel, cell by cell (choose_variant / kernel_of in pvt_trace.hip).

Rows: the kinds of scene that choose a family.  Columns: tally and history launches, given rays and device emission, and
the three placements of the scene tables (`PVT_TABLES` unset, "heads", "global").  Every cell asserts the family that
`launch_info()["variant"]` names -- FAMILY below, a literal table -- and that the launch agrees with the CPU referee under
the rule of tests/test_gpu_parity.py: every integer and every double bit for bit, the moment sums to 1e-12 relative.

The launches go through `native.DeviceScene` (pvt_trace_device_capture), the entry that reports the family of the launch
it just ran; the host-buffer entry behind test_gpu_parity.gpu_and_oracle keeps its scene to itself and refuses the
extension scenes.  The referee knows neither roughness nor captures.  A captured recorder changes no history, so that
scene is held to the referee as it stands; the rough node sits inside a shell that absorbs within 4e-8 cm (no photon
reaches it: the scene runs the rough kernels, and its histories are those of the referee's smooth scene).

`PVT_NO_LEAN` is read when a scene is created and `PVT_TABLES` at every plan of a launch, so each setting runs in a fresh
child process (this file, run as a script, is the worker) under its own time limit; a setting is only started when the
one before has ended well.  The test process itself never opens the GPU: it computes the referee's side, once.

No setting of the tables is refused for a mesh scene: the LDS plan never asks for the heads alone there ("heads" gives
it "global"), so the family table has no error cell."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAYS, SEED, RAY_SEED, EMIT_SEED, MAXSTEPS, MAX_EVENTS = 2048, 42, 123, 77, 1000, 16
TALLY_KEYS = ("rec_distinct", "rec_crossings", "rec_sums", "rec_bins")
LAUNCHES = ("tally", "history")          # record_every 0 / 1
RAYS = ("given", "device")
SETTINGS = {"unset": {}, "heads": {"PVT_TABLES": "heads"}, "global": {"PVT_TABLES": "global"}, "no_lean": {"PVT_NO_LEAN": "1"}}
# the family each row runs under each setting, as the library chose before the choice had one owner
FAMILY = {
    "box_constant": {"unset": "lean", "heads": "w4", "global": "w4", "no_lean": "w4"},
    "box_linspace": {"unset": "lean", "heads": "w4", "global": "w4", "no_lean": "w4"},
    "recorders_65": {"unset": "w4", "heads": "w4", "global": "w4"},
    "node_grid": {"unset": "grid", "heads": "w4", "global": "w4"},
    "mesh_cube": {"unset": "mesh", "heads": "mesh", "global": "mesh"},
    "rough_node": {"unset": "rough", "heads": "rough", "global": "rough"},
    "captured": {"unset": "rough", "heads": "rough", "global": "rough"},
}
CELLS = [(setting, row) for row, by_setting in FAMILY.items() for setting in by_setting]


# -- the rows ---------------------------------------------------------------------------------------------------------
def box_constant():
    """tests/scenes.py's bench_slab with constant spectra only: the lean family's EVEN kernels."""
    from pvtrace_amd import Absorber
    from tests import scenes

    scene = scenes.bench_slab(recorders=True)
    scene.root.children[0].geometry.material.components = [Absorber(0.3, name="background")]
    return scene


def box_linspace():
    """... with its dye on np.linspace(300, 1000, 200), even only up to rounding: the lean kernels that search."""
    from tests import scenes

    return scenes.bench_slab(recorders=True)


def recorders_65():
    from tests.test_gpu_parity import _scene_with_many_recorders

    return _scene_with_many_recorders(65)


def node_grid():
    """3 x 3 tiles and the world: ten nodes (28 recorders), the smallest of the tile arrays that is filed under a node grid."""
    from benchmarks.configs import tiles_lsc

    return tiles_lsc(3, recorders="all")


def mesh_cube():
    from pvtrace_amd import Absorber, Light, Material, Mesh, Node, Scene, Sphere
    from pvtrace_amd.engine import Recorder
    from pvtrace_amd.material import Cone

    world = Node(name="world", geometry=Sphere(100.0, material=Material(refractive_index=1.0)))
    path = os.path.join(ROOT, "tests", "golden", "spec_data", "20mm-xyz-cube.stl")
    cube = Node(name="cube", parent=world, geometry=Mesh.from_file(path, material=Material(
        refractive_index=1.5, components=[Absorber(0.02, name="tint")])))
    cube.rotate(0.3, (0.2, 1.0, 0.1))
    cube.recorders = [Recorder("in", event="entering"), Recorder("out", event="escaping"), Recorder("lost", event="lost")]
    lamp = Node(name="lamp", parent=world, light=Light(direction=Cone(0.2), name="lamp"))
    lamp.location = (1.0, -2.0, -40.0)
    return Scene(world)


def rough_node():
    from pvtrace_amd import Absorber, Box, FresnelSurfaceDelegate, Material, Node, Surface

    scene = box_constant()
    shell = Node(name="shell", parent=scene.root, geometry=Box((1.0, 1.0, 1.0), material=Material(
        refractive_index=1.0, components=[Absorber(1e9, name="black")])))
    shell.location = (0.3, 0.2, 3.0)     # in the beam that leaves the slab's top
    Node(name="rough", parent=shell, geometry=Box((0.5, 0.5, 0.5), material=Material(
        refractive_index=1.5, surface=Surface(FresnelSurfaceDelegate(roughness=0.3)))))
    return scene


def captured():
    scene = box_constant()
    next(r for r in scene.root.children[0].recorders if r.name == "lost").capture = 4096
    return scene


BUILDERS = {"box_constant": box_constant, "box_linspace": box_linspace, "recorders_65": recorders_65, "node_grid": node_grid,
            "mesh_cube": mesh_cube, "rough_node": rough_node, "captured": captured}


@functools.lru_cache(maxsize=None)
def prepared(row):
    from pvtrace_amd.engine import compile_scene
    from pvtrace_amd.engine.emit import EmitterTables

    scene = BUILDERS[row]()
    return scene, compile_scene(scene), EmitterTables(scene)


def rays_of(row, rays):
    """The rays of a cell on the host: the scene's lights sampled by the host emitter, or by the referee's mirror of the
    device emitter."""
    from oracle import oracle as O
    from pvtrace_amd.engine.emit import emit_bundle

    scene, _, emitter = prepared(row)
    if rays == "device":
        return O.emit(emitter, N_RAYS, emit_seed=EMIT_SEED)
    return emit_bundle(scene, N_RAYS, seed=RAY_SEED)[:3]


# -- the GPU's side: one child process per setting -----------------------------------------------------------------------
def _worker(setting, out_path):
    import torch

    from pvtrace_amd.engine import native

    out = {}
    dev = torch.device("cuda", 0)
    for row in FAMILY:
        if setting not in FAMILY[row]:
            continue
        _, compiled, emitter = prepared(row)
        dscene = native.DeviceScene(compiled, device=0, emitter=emitter)
        try:
            for launch in LAUNCHES:
                for rays in RAYS:
                    given = None if rays == "device" else tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in rays_of(row, rays))
                    every = 1 if launch == "history" else 0
                    tallies = dscene.new_tallies()
                    log = dscene.new_event_log(N_RAYS, every, MAX_EVENTS) if every else None
                    dscene.trace(given, N_RAYS, SEED, tallies, log=log, emit_seed=EMIT_SEED, record_every=every,
                                 maxsteps=MAXSTEPS, max_events=MAX_EVENTS)
                    tag = f"{row}/{launch}/{rays}"
                    out[f"{tag}/variant"] = np.array(dscene.launch_info()["variant"])
                    if every:
                        cols = dscene.new_event_columns(N_RAYS, every, MAX_EVENTS)
                        dscene.unpack_records(log, cols, N_RAYS, MAX_EVENTS, prefill=True)
                        out[f"{tag}/counts"] = log["counts"][:N_RAYS].cpu().numpy()   # (the unpack pass reads them, it does not copy them)
                        for key, _, width in native.EVENT_LOG_COLUMNS:
                            col = cols[key].cpu().numpy()
                            out[f"{tag}/{key}"] = col.reshape(-1, 3) if width == 3 else col
                    for key, value in tallies.host(0).items():
                        out[f"{tag}/{key}"] = value
        finally:
            dscene.close()
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dispatch")
    results = {}
    for setting, switches in SETTINGS.items():   # (a fault fails the fixture: the next setting is not started)
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        for name in ("PVT_TABLES", "PVT_NO_LEAN"):
            env.pop(name, None)
        env.update(switches)
        path = str(tmp / f"{setting}.npz")
        done = subprocess.run([sys.executable, os.path.abspath(__file__), setting, path], cwd=ROOT, env=env, timeout=300,
                              capture_output=True, text=True)
        assert done.returncode == 0, (setting, done.returncode, done.stderr[-2000:])
        results[setting] = dict(np.load(path))
    return results


# -- the referee's side, once per (row, launch, rays) -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def referee(row, launch, rays):
    from oracle import oracle as O

    pos, dirs, wl = rays_of(row, rays)
    return O.trace_bundle(prepared(row)[1], pos, dirs, wl, SEED, MAXSTEPS, MAX_EVENTS, 0, 4, 1 if launch == "history" else 0,
                          math_mode=O.MATH_PORTABLE)


def test_the_rows_are_what_they_are_named_for():
    """Host only: which rows the library proves plain (and which of those even), which it files under a node grid, which
    carry an extension -- the facts the families of FAMILY follow from."""
    from pvtrace_amd.engine import compile_scene, native
    from tests.test_gpu_parity import _scene_with_many_recorders

    kinds = {row: native.lean_kind(prepared(row)[1]) for row in FAMILY}
    # (a 65th recorder alone takes a scene out of the plain kind: the four-word first-crossing mask)
    assert kinds["box_constant"] == 2 and kinds["box_linspace"] == 1 and kinds["recorders_65"] == 0
    assert native.lean_kind(compile_scene(_scene_with_many_recorders(64))) == 1
    grids = {row for row in FAMILY if native.node_grid_plan(prepared(row)[1]) is not None}
    assert grids == {"node_grid"}
    assert prepared("recorders_65")[1].rec_node.shape[0] == 65
    assert prepared("rough_node")[1].has_roughness and prepared("captured")[1].has_captures
    assert not any(prepared(row)[1].has_roughness or prepared(row)[1].has_captures for row in FAMILY if row not in ("rough_node", "captured"))


@pytest.mark.gpu
@pytest.mark.parametrize("setting,row", CELLS, ids=[f"{row}-{setting}" for setting, row in CELLS])
def test_every_cell_runs_its_family_and_equals_the_referee(gpu, setting, row):
    from tests.util import assert_bundles_identical

    for launch in LAUNCHES:
        for rays in RAYS:
            tag = f"{row}/{launch}/{rays}"
            got = {k[len(tag) + 1:]: v for k, v in gpu[setting].items() if k.startswith(tag + "/")}
            assert str(got.pop("variant")) == FAMILY[row][setting], (setting, tag)
            cpu = referee(row, launch, rays)
            want = cpu if launch == "history" else {k: cpu[k] for k in TALLY_KEYS}
            assert_bundles_identical(got, want, sums_rtol=1e-12, what=f"{setting} {tag}")
            assert int(cpu["rec_crossings"].sum()) > N_RAYS // 4, tag   # the rays do meet the recorders
            if launch == "history":
                assert int(cpu["counts"].min()) >= 2 and int(cpu["counts"].max()) > 3


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
