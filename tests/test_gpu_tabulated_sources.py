"""Tabulated sources on the GPU: the kernel's emitter (`emit_one`, compiled into `emit_kernel`, `emit_chunk` and
`emit_chunk_park`) on position grids and direction tables against the float64 restatement of the two rules
(tests/exact_sources.py), bit for bit and ray for ray.  The restatement is held to the exact rule within derived bounds
on the CPU (tests/test_tabulated_sources.py), so equality with it places every device value within those bounds too.

  * `DeviceScene.emit` on every case of the table: 4 096 + 37 rays (a partial last block) at ray_offset 1 000;
  * the GENERATE rows of a history launch (`emit_chunk`) and the integer tallies of a parking stream against the referee
    on the restatement's rays (`emit_chunk_park`), reached as tests/test_gpu_emission_exact.py reaches them;
  * end to end: a scene with an image-and-table light keeps device emission, and the `origin_x` x `origin_y` heatmap
    over its terminal recorders is the histogram of the restated launch positions, integer for integer; two shards on
    one GPU give the one-rank job's tallies;
  * `pvt_scene_set_emitter` and `pvt_trace_bundle` refuse the two new type words.
"""
import math

import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd import DirectionTable, Light, Node, PositionGrid, ScatterLobe
from pvtrace_amd.engine import Heatmap, Recorder, Session, _kernel, compile_scene, native, simulate
from pvtrace_amd.engine.tally import _Probe
from tests import exact_emission as X
from tests import exact_sources as S
from tests import scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bare():
    from pvtrace_amd import Box, Material, Scene
    world = Node(name="world", geometry=Box((64.0, 64.0, 64.0), material=Material(refractive_index=1.0)))
    Node(name="block", parent=world, geometry=Box((2.0, 2.0, 2.0), material=Material(refractive_index=1.5)))
    return compile_scene(Scene(world))


# ------------------------------------------------------------------------------------------------ emit_kernel
@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_device_emission_equals_the_restatement(bare, case):
    lights = case.tables.n_lights
    assert case.n == 4096 + 37 and case.ray_offset != 0 and (lights == 1 or case.ray_offset % lights != 0)
    want = case.kernel()[:3]
    dscene = native.DeviceScene(bare, device=0, emitter=case.tables)
    try:
        got = tuple(t.cpu().numpy() for t in dscene.emit(case.n, case.emit_seed, ray_offset=case.ray_offset))
    finally:
        dscene.close()
    for g, w, what in zip(got, want, ("position", "direction", "wavelength")):
        assert np.array_equal(g, w), (case.name, what, int((g != w).sum()))


# ------------------------------------------------------------------------------------------------ emit_chunk
def test_generate_rows_of_a_history_launch_equal_the_restatement():
    from tests.test_gpu_emission_exact import block_scene, generate_rows
    case = S.BY_NAME["R-three-lights"]
    n = 4096
    pos, dirs, wl, info = generate_rows(block_scene()[0], case.tables, n, case.emit_seed, case.ray_offset)
    assert info["variant"] in ("lean", "w4"), info
    want = case.kernel()
    assert np.array_equal(wl, want[2][:n]) and np.array_equal(pos, want[0][:n]) and np.array_equal(dirs, want[1][:n])


# ------------------------------------------------------------------------------------------------ emit_chunk_park
def test_a_parking_stream_tallies_the_restatements_rays():
    from benchmarks.configs import tiles_lsc
    from tests.test_gpu_park_variant import MAXSTEPS, PARK, SEED as PARK_SEED, USUAL, assert_equal_tallies, run_stream

    # the three lights moved above the tile, shining down on it: most rays meet the slab
    lights = []
    for light in S.ROUND_ROBIN:
        light = dict(light)
        m = np.eye(4)
        m[:3, :3] = X.rotation(math.pi, (1.0, 0.0, 0.0)) @ X.rotation(0.2, (0.3, 1.0, 0.1))
        m[:3, 3] = (0.1, -0.2, 4.0)
        light["pose"] = m
        lights.append(light)
    tables = S.SourceTables(lights)
    compiled = compile_scene(tiles_lsc(1))
    sizes, emit_seed, offset = (2048,) * 4, 2 ** 64 - 3000, 0
    pos, dirs, wl, _, _ = S.kernel_bundle(tables, sum(sizes), emit_seed, offset)
    dscene = native.DeviceScene(compiled, device=0, emitter=tables)
    try:
        carried, entries, _, _ = run_stream(dscene, None, sizes, carry=True, depth=1, emit_seed=emit_seed)
    finally:
        dscene.close()
    cpu = O.trace_bundle(compiled, pos, dirs, wl, PARK_SEED, MAXSTEPS, 128, 0, 8, 0, math_mode=O.MATH_PORTABLE)
    assert entries == [PARK] * 3 + [USUAL]
    assert cpu["rec_distinct"].sum() > 1000
    assert_equal_tallies(carried, cpu, "a parking stream against the referee on the restatement's rays")


# ------------------------------------------------------------------------------------------------ end to end
TERMINAL = ("lost", "killed", "reacted", "detected")
HALF, CELLS = 2.0, 8


def shaded_scene():
    """The 5 x 5 x 1 cm slab under a half-shaded 16 x 16 image with an LED-like direction table, every terminal recorder
    with the launch-position heatmap."""
    scene = scenes.lsc_equivalent(recorders=False)
    image = np.random.default_rng(6).uniform(0.2, 1.0, (16, 16))
    image[:8, :] = 0.0
    lamp = next(n for n in scene.root.preorder() if getattr(n, "light", None) is not None)
    lamp.light = Light(position=PositionGrid(image, (-HALF, -HALF, None), (HALF, HALF, None)),
                       direction=DirectionTable(ScatterLobe.gaussian(10.0, "normal", nodes=257).table), name=lamp.light.name)
    fresh = lambda: [Heatmap("origin_x", "origin_y", (-HALF, HALF, CELLS), (-HALF, HALF, CELLS))]
    names = []
    for n in scene.root.preorder():
        if n.geometry is None:
            continue
        n.recorders = [Recorder(f"{event}-{n.name}", event=event, histograms=fresh()) for event in TERMINAL]
        names += [rec.name for rec in n.recorders]
    scene.root.recorders = list(scene.root.recorders) + [Recorder("exit", event="exit", histograms=fresh())]
    return scene, names + ["exit"], fresh()[0]


def test_an_image_and_table_light_keeps_device_emission_and_its_origins_are_the_restatements():
    scene, names, axes = shaded_scene()
    n, seed, emit_seed = 4096, 5, 31
    with Session(scene) as s:
        assert s.emission == "device"                    # ("host" before the feature: the silent fallback)
        tables = s.emitter
        result = s.collect(s.submit(n, seed, record_every=0, emit_seed=emit_seed))
    pos = S.kernel_bundle(tables, n, emit_seed, 0)[0]
    ix, iy = _Probe._bin_indices(pos[:, 0], axes.a), _Probe._bin_indices(pos[:, 1], axes.b)
    assert ix.min() >= 0 and iy.min() >= 0
    want = np.bincount(ix * axes.b.bins + iy, minlength=axes.size)
    # (the lamp is turned about x: the image's shaded half is one half of the face, and only that half is empty)
    assert np.count_nonzero(want) == CELLS * CELLS // 2
    recs = [result.recorders[name] for name in names]
    assert sum(rec.rays for rec in recs) == n
    assert np.array_equal(sum(np.asarray(rec._bins[0]) for rec in recs), want)


def test_two_shards_give_the_one_rank_jobs_tallies():
    from tests.test_gpu_history_counters import same_tallies, tallies_of
    scene, _, _ = shaded_scene()
    n, seed, emit_seed = 4096, 13, 21
    whole = tallies_of(simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed).data)
    sharded = simulate(scene, n, seed=seed, record_every=0, emission="device", emit_seed=emit_seed, devices=[0, 0])
    same_tallies(whole, tallies_of(sharded.data), "two shards")
    assert np.asarray(whole["rec_bins"]).sum() == n          # every photon ends in one terminal recorder's heatmap


# ------------------------------------------------------------------------------------------------ the older entries
@pytest.mark.parametrize("word", ["position", "direction"])
def test_the_entries_without_source_tables_refuse_the_new_type_words(bare, word):
    tables = X.Tables([dict(pos=(4, (0.0, 0.0, 0.0)))] if word == "position" else [dict(dir=(5, 0.0))])
    with pytest.raises(ValueError, match="emitter type out of range"):
        native.DeviceScene(bare, device=0, emitter=tables)
    with pytest.raises(ValueError, match="emitter type out of range"):
        _kernel.trace_bundle(bare, None, None, 64, 1, 100, 8, 0, 1, 0, emitter=tables, emit_seed=3)
