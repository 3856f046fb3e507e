"""Tabulated sources on the CPU: `PositionGrid` and `DirectionTable` (a wrapped `PhaseFunctionTable`), their lowering
(`engine/emit.py`), the packer's validation (`pvt_sources_check`) and the host sampler, against the references of
tests/exact_sources.py.

  * every refusal of `PositionGrid` has its message, and the packer refuses the same problem in the same words;
  * the CDF is built as the contract states; `classify_*` recognise the delegates; `EmitterTables(scene, strict=True)`
    carries the pooled tables (on the commit before the feature it raised);
  * the float64 restatement lies within the exact rule's derived bound for every ray of every case;
  * each planted fault moves rays of a named case beyond that bound, decided from the references alone;
  * the host sampler takes the contract's draws in its order and lies within the bound of ITS operations; its cell
    occupancy over 2 10^5 samples passes a chi-square against the weights (p > 10^-6) under a fixed seed, and fails it
    with the slot order transposed in a scratch copy;
  * the resident-scene key covers the tables' bytes.
"""
import copy
import math
from fractions import Fraction as F

import mpmath
import numpy as np
import pytest

from pvtrace_amd import (
    Box, CoatingPattern, ConcentrationGrid, DirectionTable, Light, Material, Node, PhaseFunctionTable, PositionGrid, ScatterLobe, Scene,
    VolumeMap,
)
from pvtrace_amd.engine import compile_scene, emit as host, native
from pvtrace_amd.engine.compiler import UnsupportedSceneError
from pvtrace_amd.light import RectangularMask
from tests import exact_sources as S

IMG = np.arange(12.0).reshape(4, 3)


# ------------------------------------------------------------------------------------------------ refusals
def _emitter(grid_edit=None, **edits):
    """The tables of one light with a 2 x 2 x 1 grid and a two-angle table, edited -> an object `pvt_sources_check` takes."""
    grid = dict(shape=(2, 2, 1), lower=(-1.0, -1.0, None), upper=(1.0, 1.0, None), weights=[1.0, 2.0, 3.0, 4.0])
    tab = S.SourceTables([dict(grid=grid, table=S.TWO_ANGLES)])
    for name, value in edits.items():
        setattr(tab, name, np.array(value, dtype=getattr(tab, name).dtype))
    if grid_edit:
        grid_edit(tab)
    return tab


def _set(name, index, value):
    def edit(tab):
        getattr(tab, name)[index] = value
    return edit


SHARED_REFUSALS = {
    # the problem: (what PositionGrid is given, the same problem in the packed tables, the words both use)
    "negative weight": (lambda: PositionGrid([[1.0, -1.0]], (0, 0, None), (1, 1, None)),
                        _set("grid_cdf", 2, 0.05), "position grid: weights must be finite and >= 0"),
    "infinite weight": (lambda: PositionGrid([[1.0, math.inf]], (0, 0, None), (1, 1, None)),
                        _set("grid_cdf", 2, math.nan), "position grid: weights must be finite and >= 0"),
    "too many cells": (lambda: PositionGrid(np.ones((2049, 2049)), (0, 0, None), (1, 1, None)),
                       _set("grid_shape", (0, 0), 3000000), "position grid: more than 2^22 cells"),
    "unbounded axis of several cells": (lambda: PositionGrid(IMG, (0, None, None), (1, None, None)),
                                        _set("grid_bounded", (0, 1), 0), "position grid: only an axis with one cell may be unbounded"),
    "infinite bound": (lambda: PositionGrid(IMG, (0, -math.inf, None), (1, 1, None)),
                       _set("grid_lower", (0, 1), -math.inf), "position grid: lower and upper must be finite"),
    "nan bound": (lambda: PositionGrid(IMG, (0, 0, None), (math.nan, 1, None)),
                  _set("grid_h", (0, 0), math.nan), "position grid: lower and upper must be finite"),
    "empty axis": (lambda: PositionGrid(IMG, (0, 1, None), (1, 1, None)),
                   _set("grid_h", (0, 1), 0.0), "position grid: needs lower < upper on each axis"),
    "reversed axis": (lambda: PositionGrid(IMG, (0, 1, None), (1, -1, None)),
                      _set("grid_h", (0, 1), -1.0), "position grid: needs lower < upper on each axis"),
    "no cell on an axis": (lambda: PositionGrid(np.zeros((3, 0, 1)), (0, 0, None), (1, 1, None)),
                           _set("grid_shape", (0, 1), 0), "position grid: shape must be >= 1 on each axis"),
}


@pytest.mark.parametrize("problem", sorted(SHARED_REFUSALS))
def test_the_class_and_the_packer_refuse_in_the_same_words(built, problem):
    make, edit, words = SHARED_REFUSALS[problem]
    with pytest.raises(ValueError) as raised:
        make()
    assert str(raised.value).startswith(words), str(raised.value)
    assert native.sources_check(_emitter(edit)) == words


def test_the_other_refusals_of_the_class_have_their_own_messages():
    messages = {}
    for problem, make in {
        "sum": lambda: PositionGrid(np.zeros((2, 2)), (0, 0, None), (1, 1, None)),
        "sum overflows": lambda: PositionGrid(np.full((2, 2), 1e308), (0, 0, None), (1, 1, None)),
        "dimensions": lambda: PositionGrid(np.ones(4), (0, 0, None), (1, 1, None)),
        "dtype": lambda: PositionGrid([["a", "b"]], (0, 0, None), (1, 1, None)),
        "one None": lambda: PositionGrid(IMG, (0, 0, None), (1, 1, 2.0)),
        "tuples": lambda: PositionGrid(IMG, (0, 0), (1, 1)),
    }.items():
        with pytest.raises(ValueError) as raised:
            make()
        messages[problem] = str(raised.value)
        assert messages[problem].startswith("position grid: "), messages[problem]
    assert messages["sum"] == messages["sum overflows"] == "position grid: the sum of the weights must be positive and finite"
    assert len(set(messages.values())) == 5
    assert not any(m.startswith(words) for m in messages.values() for _, _, words in SHARED_REFUSALS.values())


PACKER_REFUSALS = {
    "accepted": (None, None),
    "grid word without sources": (lambda tab: (setattr(tab, "n_grids", 0), setattr(tab, "n_tables", 0)), "emitter type out of range"),
    "unknown position word": (_set("pos_type", 0, 5), "emitter type out of range"),
    "unknown direction word": (_set("dir_type", 0, 6), "emitter type out of range"),
    "negative word": (_set("wl_type", 0, -1), "emitter type out of range"),
    "grid not named": (_set("light_grid", 0, -1), "source tables: a light names a grid exactly when it is tagged PVT_POS_GRID"),
    "table named by a built-in": (_set("dir_type", 0, 0), "source tables: a light names a table exactly when it is tagged PVT_DIR_TABLE"),
    "missing grid": (_set("light_grid", 0, 1), "source tables: light names a missing grid"),
    "missing table": (_set("light_table", 0, 3), "source tables: light names a missing table"),
    "cdf range": (_set("grid_cdf_start", 0, 1), "position grid: CDF range out of bounds"),
    "cdf ends": (_set("grid_cdf", 4, 0.99), "position grid: the CDF must run from exactly 0 to exactly 1"),
    "cdf start": (_set("grid_cdf", 0, -0.5), "position grid: the CDF must run from exactly 0 to exactly 1"),
    "mu ends": (_set("table_mu", 0, -0.5), "direction table: the mu axis must run from exactly -1 to exactly 1"),
    "table cdf ends": (_set("table_cdf", 1, 0.5), "direction table: every CDF row must run from exactly 0 to exactly 1"),
    "table range": (_set("table_nmu", 0, 3), "direction table: wavelength, mu or CDF range out of bounds"),
}


@pytest.mark.parametrize("problem", sorted(PACKER_REFUSALS))
def test_the_packer_validates_the_tables_without_a_gpu(built, problem):
    edit, words = PACKER_REFUSALS[problem]
    assert native.sources_check(_emitter(edit)) == words


def test_the_packer_accepts_every_case_and_the_built_ins_alone(built):
    for case in S.CASES:
        assert native.sources_check(case.tables) is None, case.name
    from tests import exact_emission as X
    assert native.sources_check(X.BY_NAME["R-seven-lights"].tables) is None


# ------------------------------------------------------------------------------------------------ the class
def test_the_cdf_is_built_as_stated():
    rng = np.random.default_rng(4)
    for weights in (rng.uniform(0.0, 1.0, (4, 2, 3)), S._image()[:, :, 0], [[0.0, 3.0]], rng.integers(0, 3, (3, 3, 1))):
        flat = np.ndim(weights) == 2 or np.shape(weights)[2] == 1
        grid = PositionGrid(weights, (0, 0, None if flat else 0), (1, 1, None if flat else 1))
        want = S.running_cdf(weights)
        assert grid.cdf.tolist() == want and want[0] == 0.0 and want[-1] == 1.0
        assert grid.cdf.size == grid.weights.size + 1
    grid = PositionGrid(IMG, (-2.0, -0.3, None), (2.0, 0.4, None))
    assert grid.shape == (4, 3, 1) and grid.bounded == (True, True, False)
    assert grid.h == ((2.0 - -2.0) / 4.0, (0.4 - -0.3) / 3.0, 1.0)
    np.random.seed(3)
    p = grid()
    assert isinstance(p, tuple) and len(p) == 3 and p[2] == 0.0 and -2.0 <= p[0] < 2.0 and -0.3 <= p[1] < 0.4
    bundle = grid.sample(1000)
    assert bundle.shape == (1000, 3) and not bundle[:, 2].any()
    assert not np.any((bundle[:, 0] < -1.0) & (bundle[:, 1] < -0.3 + 0.7 / 3.0))     # cell (0, 0) has weight 0


def test_like_takes_the_lattice_of_its_owner():
    field = ConcentrationGrid(np.arange(24.0).reshape(2, 3, 4), (-1, -2, -3), (1, 2, 3))
    grid = PositionGrid.like(field)
    assert grid.lattice.same(field.lattice) and np.array_equal(grid.weights, field.values)
    vmap = VolumeMap("absorbed", shape=(2, 3, 4), lower=(-1, -2, -3), upper=(1, 2, 3))
    assert PositionGrid.like(vmap, np.ones((2, 3, 4))).lattice.same(vmap.lattice)
    pattern = CoatingPattern(np.ones((2, 3, 1)), (-1, -2, None), (1, 2, None))
    flat = PositionGrid.like(pattern)
    assert flat.bounded == (True, True, False) and flat.lower[:2] == (-1.0, -2.0) and flat.shape == (2, 3, 1)
    with pytest.raises(ValueError, match="owner's shape"):
        PositionGrid.like(field, np.ones((2, 3)))
    with pytest.raises(ValueError, match="has no lattice"):
        PositionGrid.like(object(), np.ones((2, 3, 4)))


# ------------------------------------------------------------------------------------------------ the lowering
def _scene(*lights, turn=True):
    world = Node(name="world", geometry=Box((40.0, 40.0, 40.0), material=Material(refractive_index=1.0)))
    for k, light in enumerate(lights):
        node = Node(name=f"light-{k}", parent=world, light=light)
        node.location = (0.1 * k, -0.2, 3.0)
        if turn:
            node.rotate(0.7 + k, (0.3, -1.0, 0.6))
    return Scene(world)


def _product_lights():
    image = PositionGrid(S._image()[:, :, 0], (-2.5, -2.5, None), (2.5, 2.5, None))
    block = PositionGrid(S.GRID_423["weights"], S.GRID_423["lower"], S.GRID_423["upper"])
    led = DirectionTable(ScatterLobe.gaussian(10.0, "normal", nodes=257).table)
    rows = DirectionTable(PhaseFunctionTable(S._A3, [np.exp(-0.5 * (S._A3 / 15.0) ** 2), np.exp(-0.5 * (S._A3 / 40.0) ** 2),
                                                      1.0 + 0.0 * S._A3], wavelength=[450.0, 550.0, 700.0]))
    return image, block, led, rows


def test_classify_recognises_the_delegates():
    image, block, led, rows = _product_lights()
    assert host.classify_position(image) == (host.POS_GRID, image) and host.POS_GRID == 4
    assert host.classify_direction(rows) == (host.DIR_TABLE, rows.table) and host.DIR_TABLE == 5
    assert host.classify_direction(rows.table) is None        # a bare table stays the user delegate it always was
    with pytest.raises(ValueError, match="must be a PhaseFunctionTable"):
        DirectionTable(lambda: (0.0, 0.0, 1.0))
    np.random.seed(2)
    one, many = np.asarray(rows()), rows.sample(50)
    assert one.shape == (3,) and many.shape == (50, 3) and np.allclose((many * many).sum(axis=1), 1.0)
    assert host.classify_position(RectangularMask(1.0, 2.0))[0] == host.POS_RECT
    assert host.classify_position(lambda: (0.0, 0.0, 0.0)) is None


def test_strict_emitter_tables_carry_the_pooled_tables():
    image, block, led, rows = _product_lights()
    again = PositionGrid(S._image()[:, :, 0], (-2.5, -2.5, None), (2.5, 2.5, None))      # equal bytes: stored once
    scene = _scene(Light(position=image, direction=led), Light(position=RectangularMask(1.0, 2.0)),
                   Light(position=block, direction=rows), Light(position=again, direction=rows))
    tab = host.EmitterTables(scene, strict=True)         # (raised UnsupportedSceneError before the feature)
    assert all(tab.builtin) and tab.has_sources
    assert tab.pos_type.tolist() == [4, 1, 4, 4] and tab.dir_type.tolist() == [5, 0, 5, 5]
    assert tab.light_grid.tolist() == [0, -1, 1, 0] and tab.light_table.tolist() == [0, -1, 1, 1]
    assert tab.n_grids == 2 and tab.n_tables == 2
    assert tab.grid_shape.tolist() == [[64, 64, 1], [4, 2, 3]] and tab.grid_bounded.tolist() == [[1, 1, 0], [1, 1, 1]]
    assert tab.grid_cdf_start.tolist() == [0, 4097] and tab.grid_cdf.size == 4097 + 25
    assert np.array_equal(tab.grid_cdf[4097:], block.cdf) and np.array_equal(tab.grid_h[1], block.lattice.h)
    assert tab.table_nw.tolist() == [1, 3] and tab.table_nmu.tolist() == [257, 19]
    assert tab.table_wl_start.tolist() == [0, 1] and tab.table_wavelength.tolist() == [0.0, 450.0, 550.0, 700.0]
    assert np.array_equal(tab.table_cdf[257:], rows.table.cdf.reshape(-1)) and np.array_equal(tab.table_mu[257:], rows.table.mu)
    with pytest.raises(UnsupportedSceneError):
        host.EmitterTables(_scene(Light(position=lambda: (0.0, 0.0, 0.0), direction=led)), strict=True)
    with pytest.raises(UnsupportedSceneError):           # a bare table is not lowered: wrapping it is what asks for that
        host.EmitterTables(_scene(Light(position=image, direction=led.table)), strict=True)


def test_the_packer_accepts_the_lowered_tables(built):
    image, block, led, rows = _product_lights()
    tab = host.EmitterTables(_scene(Light(position=image, direction=led), Light(position=block, direction=rows)), strict=True)
    assert native.sources_check(tab) is None


def test_the_resident_scene_key_covers_the_tables_bytes():
    from pvtrace_amd.engine import api
    image, _, led, _ = _product_lights()
    other = np.array(image.weights[:, :, 0])
    other[40, 40] *= 1.5
    scenes = [_scene(Light(position=g, direction=led)) for g in
              (image, PositionGrid(other, (-2.5, -2.5, None), (2.5, 2.5, None)),
               PositionGrid(image.weights[:, :, 0], (-2.5, -2.5, None), (2.5, 2.5, None)))]
    keys = [api._scene_key(compile_scene(s), host.EmitterTables(s, strict=True), 0) for s in scenes]
    assert keys[0] != keys[1] and keys[0] == keys[2]
    led2 = DirectionTable(ScatterLobe.gaussian(11.0, "normal", nodes=257).table)
    s = _scene(Light(position=image, direction=led2))
    assert api._scene_key(compile_scene(s), host.EmitterTables(s, strict=True), 0) != keys[0]


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("case", S.CASES, ids=[c.name for c in S.CASES])
def test_the_restatement_lies_within_the_exact_rules_bound(case):
    pos, dirs, wl, draws, infos = case.kernel()
    refs = case.exact()
    assert all(ref["draws"] == k and ref["slot"] == info["slot"] and ref["segment"] == info["segment"]
               for ref, k, info in zip(refs, draws, infos))
    worst = S.worst_ratio(refs, pos, dirs, wl)
    print(f"{case.name}: worst |restatement - exact| / bound = {worst:.3f}")
    assert worst <= 1.0                                                  # every ray, none excused


def test_the_cases_reach_what_they_name():
    slots = lambda name: [info["slot"] for info in S.BY_NAME[name].kernel()[4]]
    assert set(slots("G-1x1x1")) == {0} and set(slots("G-2x1x1-zero-cell")) == {1}
    ties = S.BY_NAME["G-3x3x1-ties"]
    assert set(slots("G-3x3x1-ties")) == {1, 2, 4, 5, 6, 7}              # the zero cells 0, 3 and 8 are never chosen
    cdf = ties.tables.grid_cdf.tolist()
    first = [S.stream(S.emit_key(ties.emit_seed, ties.ray_offset + i), 1)[0] for i in range(ties.n)]
    assert sum(u in cdf for u in first) >= 5 and cdf[3] in first         # rays ON a knot, one on the tie
    assert set(slots("G-4x2x3")) == set(range(24))
    weights = S._image().reshape(-1)
    assert len(set(slots("G-64x64-image"))) > 1000 and all(weights[s] > 0.0 for s in slots("G-64x64-image"))
    segs = lambda name: {info["segment"] for info in S.BY_NAME[name].kernel()[4]}
    assert segs("T-two-angles") == {0}
    nm = len(S.ZERO_MASS[1])
    row = S.ZERO_MASS[2][0]
    empty = {j for j in range(nm - 1) if row[j + 1] == row[j]}
    assert empty and not (segs("T-zero-mass") & empty) and segs("T-zero-mass") == set(range(nm - 1)) - empty
    assert set(S.BY_NAME["T-three-rows"].kernel()[3]) == {3} and set(S.BY_NAME["T-two-angles"].kernel()[3]) == {2}
    robin = S.BY_NAME["R-three-lights"]
    assert robin.ray_offset % 3 != 0 and {(info["light"], int(k)) for info, k in zip(robin.kernel()[4], robin.kernel()[3])} == \
        {(0, 2), (1, 5), (2, 6)}


FAULT_CASES = {"cell-bisect-lt": "G-3x3x1-ties", "slot-transposed": "G-4x2x3", "axis-draws-zyx": "G-4x2x3",
               "h-by-reciprocal": "G-4x2x3", "u1-not-drawn": "T-three-rows", "row-not-first": "T-three-rows"}


@pytest.mark.parametrize("fault", S.FAULTS)
def test_each_planted_fault_is_caught_by_a_named_case(fault):
    """From the references alone: the rule with the fault planted moves rays of its case, so a kernel with that fault,
    which must EQUAL the right restatement ray for ray, fails there.  Every fault but one also leaves the exact rule's
    bound.  The exception is h formed with a reciprocal: it is off by one ulp of a cell width, which no error analysis of
    three roundings can tell from a rounding -- the equality with the restatement is what sees it (818 rays move)."""
    case = S.BY_NAME[FAULT_CASES[fault]]
    pos, dirs, wl = case.kernel()[:3]
    bpos, bdirs, bwl, _, _ = S.kernel_bundle(case.tables, case.n, case.emit_seed, case.ray_offset, fault=fault)
    moved = (pos != bpos).any(axis=1) | (dirs != bdirs).any(axis=1) | (wl != bwl)
    print(f"{fault}: {int(moved.sum())} rays of {case.name} move")
    assert moved.sum() >= 5      # (the fewest: a ray must sit ON a knot to see the `<`, and five of the case's do)
    if fault != "h-by-reciprocal":
        assert S.worst_ratio(case.exact(), bpos, bdirs, bwl) > 1.0
    assert set(FAULT_CASES) == set(S.FAULTS)


# ------------------------------------------------------------------------------------------------ the host sampler
def _host_light(tab, li, draws):
    calls = []

    def uniform(n):
        assert n == len(draws)
        calls.append(len(calls))
        return draws[:, calls[-1]].copy()

    pos, direc, wl = host._sample_light(tab, li, len(draws), uniform)
    return pos, direc, wl, len(calls)


def test_the_host_sampler_takes_the_contracts_draws_and_lies_within_its_bound():
    image, block, led, rows = _product_lights()
    scene = _scene(Light(position=image, direction=led), Light(position=block, direction=rows), Light(position=block))
    tab = host.EmitterTables(scene, strict=True)
    n, seed, offset = 1500, 77, 1000
    refs = [S.exact_emit(tab, seed, offset + i, host=True) for i in range(n)]
    worst = 0.0
    for li in range(tab.n_lights):
        mine = [i for i in range(n) if refs[i]["light"] == li]
        draws = np.array([S.stream(S.emit_key(seed, offset + i), 10) for i in mine])
        pos, direc, wl, calls = _host_light(tab, li, draws)
        assert all(refs[i]["draws"] == calls for i in mine)
        with mpmath.workdps(S.DIGITS):
            for j, i in enumerate(mine):
                ref = refs[i]
                pairs = [(pos[j, a], ref["local_pos"][a], ref["e_local_pos"][a]) for a in range(3)]
                pairs += [(direc[j, a], ref["local_dir"][a], ref["e_local_dir"][a]) for a in range(3)]
                for got, want, bound in pairs:
                    assert math.isfinite(got)
                    err = abs(float(S._mp(F(float(got))) - want))
                    if err > 0.0:
                        worst = max(worst, err / bound if bound > 0.0 else math.inf)
    print(f"worst |host - exact| / bound = {worst:.3f}")
    assert worst <= 1.0
    # ... and through emit_bundle: the world frame, ray i from light i mod 3, within the order-free pose bound
    p, d, w, _ = host.emit_bundle(scene, 300, seed=5)
    assert p.shape == (300, 3) and np.allclose((d * d).sum(axis=1), 1.0, atol=1e-12) and np.all(w == 555.0)


def _chi_square_p(observed, weights):
    """p of Pearson's chi-square of cell counts against weights; a count in a cell of weight 0 gives p = 0."""
    observed, weights = np.asarray(observed, dtype=np.float64).reshape(-1), np.asarray(weights, dtype=np.float64).reshape(-1)
    if observed[weights == 0.0].any():
        return 0.0
    live = weights > 0.0
    expect = observed.sum() * weights[live] / weights[live].sum()
    x2 = float(((observed[live] - expect) ** 2 / expect).sum())
    return float(mpmath.gammainc(0.5 * (live.sum() - 1), 0.5 * x2, mpmath.inf, regularized=True))


CHI_SEED = 20260
CHI_CASES = {"4x2x3": lambda: (np.where(np.arange(24).reshape(4, 2, 3) % 5 == 0, 0.0, S.GRID_423["weights"]),
                                S.GRID_423["lower"], S.GRID_423["upper"]),
             "6x5-flat": lambda: (np.random.default_rng(8).uniform(0.0, 1.0, (6, 5)) ** 2, (-1.0, 0.0, None), (1.0, 3.0, None))}


@pytest.mark.parametrize("name", sorted(CHI_CASES))
def test_the_host_samplers_cell_occupancy_follows_the_weights(name):
    weights, lower, upper = CHI_CASES[name]()
    grid = PositionGrid(weights, lower, upper)
    n = 200_000

    def occupancy(g):
        tab = host.EmitterTables(_scene(Light(position=g), turn=False), strict=True)
        np.random.seed(CHI_SEED)
        pos, _, _ = host._sample_light(tab, 0, n, lambda m: np.random.uniform(0, 1, m))
        cell = [np.floor((pos[:, a] - g.lower[a]) / g.h[a]).astype(np.int64) if g.bounded[a] else np.zeros(n, dtype=np.int64)
                for a in range(3)]
        assert all(c.min() >= 0 and c.max() < s for c, s in zip(cell, g.shape))
        counts = np.zeros(g.shape, dtype=np.int64)
        np.add.at(counts, tuple(cell), 1)
        return counts

    p = _chi_square_p(occupancy(grid), grid.weights)
    print(f"{name}: chi-square p = {p:.3g}")
    assert p > 1e-6
    wrong = copy.copy(grid)      # the slot order transposed, planted in a scratch copy of the sampler

    def transposed(uniform, m):
        k = grid.cells(uniform(m))
        index = np.unravel_index(k, grid.shape[::-1])[::-1]
        out = np.zeros((m, 3))
        for a in range(3):
            if grid.bounded[a]:
                out[:, a] = grid.lower[a] + (index[a].astype(np.float64) + uniform(m)) * grid.h[a]
        return out

    wrong.positions = transposed
    assert _chi_square_p(occupancy(wrong), grid.weights) < 1e-6
