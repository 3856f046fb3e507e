"""pvtrace_amd/lattice.py: the one lattice value, cell rule and walk that concentration fields, volume maps, path-length
maps and coating patterns share.

The referee is tests/golden/lattice_walk.npz, recorded (tests/golden/make_golden.py --lattice) from `material._march`,
`tally.path_segment_pieces`, `ConcentrationGrid.cell_of` and `pattern_cell` as they were when each carried its own copy
of the walk and of the cell rule: the shared code must reproduce it bit for bit -- cells, depths, piece units, order."""
import math
import os

import numpy as np
import pytest

from pvtrace_amd import lattice as L
from pvtrace_amd import material
from pvtrace_amd.engine.recorder import VolumeMap
from pvtrace_amd.engine.tally import path_segment_pieces
from pvtrace_amd.material import CoatingPattern, ConcentrationGrid, pattern_cell

SHAPES = ((1, 1, 1), (2, 2, 1), (3, 4, 5), (7, 1, 2))
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lattice_walk.npz"))


def case(shape):
    key = "x".join(str(n) for n in shape)
    return {name[len(key) + 1:]: GOLDEN[name] for name in GOLDEN.files if name.startswith(key + "_")}


def bits(values):
    return np.asarray(values, dtype=np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("shape", SHAPES)
def test_the_march_reproduces_the_recorded_outcomes_and_cell_order(shape):
    g = case(shape)
    assert len(g["p"]) >= 500
    grid = ConcentrationGrid(g["values"], g["lower"], g["upper"])
    for visits, count, taus in (("visits", "visit_count", g["tau"]), ("free_visits", "free_visit_count", None)):
        seen, counts, outcomes = [], [], []
        for j in range(len(g["p"])):
            mine = []

            def alpha(cell):
                mine.append(cell)
                return float(g["values"][cell])

            tau = math.inf if taus is None else float(taus[j])
            outcomes.append(material._march(grid, g["p"][j], g["u"][j], tau, float(g["length"][j]), alpha))
            seen.extend(mine)
            counts.append(len(mine))
        assert counts == g[count].tolist()
        assert seen == [tuple(c) for c in g[visits].tolist()]
        if taus is not None:
            assert [bool(o[0]) for o in outcomes] == g["absorbed"].tolist()
            assert bits([o[1] for o in outcomes]) == bits(g["depth"])
            assert [(-1, -1, -1) if o[2] is None else tuple(o[2]) for o in outcomes] == [tuple(c) for c in g["cell"].tolist()]
        else:
            assert not any(o[0] for o in outcomes)


@pytest.mark.parametrize("shape", SHAPES)
def test_the_path_pieces_reproduce_the_recorded_cells_units_and_order(shape):
    g = case(shape)
    grid = ConcentrationGrid(g["values"], g["lower"], g["upper"])
    lo, h = tuple(float(v) for v in g["lower"]), tuple(float(v) for v in grid.h)
    cells, units, counts = [], [], []
    for j in range(len(g["p"])):
        pieces = path_segment_pieces([float(v) for v in g["p"][j]], [float(v) for v in g["u"][j]], float(g["length"][j]),
                                     lo, h, shape)
        cells.extend(cell for cell, _ in pieces)
        units.extend(k for _, k in pieces)
        counts.append(len(pieces))
    assert counts == g["piece_count"].tolist()
    assert cells == [tuple(c) for c in g["piece_cells"].tolist()]
    assert units == g["piece_units"].tolist()


@pytest.mark.parametrize("shape", SHAPES)
def test_the_cell_of_a_point_reproduces_the_recorded_cells_under_each_range_rule(shape):
    g = case(shape)
    grid = ConcentrationGrid(g["values"], g["lower"], g["upper"])
    lo, hi = tuple(float(v) for v in g["lower"]), tuple(float(v) for v in g["upper"])
    assert [grid.cell_of(p) for p in g["p"]] == [tuple(c) for c in g["cell_of"].tolist()]
    bounded = CoatingPattern(g["values"], lo, hi)
    free = CoatingPattern(g["values"], tuple(None if n == 1 else v for n, v in zip(shape, lo)),
                          tuple(None if n == 1 else v for n, v in zip(shape, hi)))
    for pattern, name in ((bounded, "pattern_slot"), (free, "free_pattern_slot")):
        slots = [pattern_cell(pattern, p) for p in g["p"]]
        assert [-1 if s is None else s for s in slots] == g[name].tolist()
    # the vectorised form the event maps bin with is the same rule: inside on all axes <=> the pattern's slot exists
    h = grid.h
    inside = np.ones(len(g["p"]), dtype=bool)
    flat = np.zeros(len(g["p"]), dtype=np.int64)
    for a in range(3):
        ok, f = L.cell_inside(g["p"][:, a], lo[a], h[a], shape[a])
        inside &= ok
        flat = flat * shape[a] + np.where(ok, f, 0.0).astype(np.int64)
    assert np.array_equal(np.where(inside, flat, -1), g["pattern_slot"])


@pytest.mark.parametrize("shape", SHAPES)
def test_the_two_walk_modes_agree_on_rays_that_stay_strictly_inside_the_box(shape):
    """Inside the box the two plane sets differ only by the outer planes 0 and n, which such a ray never reaches."""
    g = case(shape)
    lo, hi = [float(v) for v in g["lower"]], [float(v) for v in g["upper"]]
    h = L.Lattice(shape, lo, hi, "test").h
    compared = 0
    for j in range(len(g["p"])):
        for scale in (1.0, 0.25):   # (the recorded lengths reach twice the box's diagonal: shortened, more rays stay inside)
            p, u, length = g["p"][j], g["u"][j], scale * float(g["length"][j])
            end = p + length * u
            if not all(lo[a] < min(p[a], end[a]) and max(p[a], end[a]) < hi[a] for a in range(3)):
                continue
            assert list(L.walk(p, u, length, lo, h, shape, slabs=False)) == list(L.walk(p, u, length, lo, h, shape, slabs=True))
            compared += 1
    assert compared >= 100


def test_the_lattice_value_validates_once_with_the_callers_label():
    ok = L.Lattice((2, 3, 4), (-1, -1, 0), (1, 2, 2), "Thing 'm'")
    assert (ok.shape, ok.lower, ok.upper, ok.h) == ((2, 3, 4), (-1.0, -1.0, 0.0), (1.0, 2.0, 2.0), (1.0, 1.0, 0.5))
    assert L.slot(ok.shape, (1, 2, 3)) == (1 * 3 + 2) * 4 + 3
    for shape, lower, upper, message in (
        ((2, 2), (0, 0, 0), (1, 1, 1), "Thing 'm': shape must be three integers"),
        ((2, 2.5, 2), (0, 0, 0), (1, 1, 1), "Thing 'm': shape must be three integers"),
        ((2, 0, 2), (0, 0, 0), (1, 1, 1), "Thing 'm': shape must be >= 1"),
        ((1, 1, 1), (0, 0), (1, 1), "Thing 'm': lower and upper must have three coordinates"),
        ((1, 1, 1), (0, 0, -math.inf), (1, 1, 1), "Thing 'm': lower and upper must be finite"),
        ((1, 1, 1), (0, 0, 0), (1, 1, math.nan), "Thing 'm': lower and upper must be finite"),
        ((1, 1, 1), (0, 2, 0), (1, 1, 1), "Thing 'm': needs lower < upper"),
        ((1, 1, 1), (0, 0, 1), (1, 1, 1), "Thing 'm': needs lower < upper"),
    ):
        with pytest.raises(ValueError, match=message):
            L.Lattice(shape, lower, upper, "Thing 'm'")


def test_same_lattice_is_bitwise_and_like_takes_anything_with_a_lattice():
    grid = ConcentrationGrid(np.ones((3, 2, 5)), (-2.0, -1.0, 0.0), (2.5, 1.0, 0.75))
    vmap = VolumeMap.like(grid, "m")
    assert vmap.lattice.same(grid.lattice) and grid.same_lattice(vmap)
    assert VolumeMap.like(vmap, "again").lattice.same(grid.lattice)
    assert CoatingPattern.like(vmap, np.ones((3, 2, 5))).lower == vmap.lower
    assert VolumeMap.like(vmap, "again").cell_widths == tuple(grid.h)
    other = ConcentrationGrid(np.ones((3, 2, 5)), (-2.0, -1.0, -0.0), (2.5, 1.0, 0.75))    # -0.0 == 0.0, other bits
    assert not grid.same_lattice(other)
    assert not grid.same_lattice(ConcentrationGrid(np.ones((3, 2, 4)), (-2.0, -1.0, 0.0), (2.5, 1.0, 0.75)))


def test_the_three_range_rules_on_the_edges_and_on_nan():
    lo, h, n = -1.0, 0.5, 4                       # planes at -1, -0.5, 0, 0.5, 1
    points = (-7.0, -1.5, -1.0, -0.25, 0.99, 1.0, 1.5, 30.0, math.inf, -math.inf, math.nan)
    assert [L.cell_clamped(p, lo, h, 0, n - 1) for p in points] == [0, 0, 0, 1, 3, 3, 3, 3, 3, 0, 0]
    assert [L.cell_clamped(p, lo, h, -1, n) for p in points] == [-1, -1, 0, 1, 3, 4, 4, 4, 4, -1, -1]
    assert [int(L.cell_inside(p, lo, h, n)[1]) if L.cell_inside(p, lo, h, n)[0] else None for p in points] == \
        [None, None, 0, 1, 3, None, None, None, None, None, None]
    assert (L.fmin(math.nan, 1.0), L.fmin(1.0, math.nan), L.fmax(math.nan, 1.0), L.fmax(1.0, math.nan)) == (1.0,) * 4
