"""The kernel's surface branch under an absorbing coating (`coat_absorb_call` and the three-way decision,
pvt_trace_kernel.h) against the float64 restatement of the PvtCoatingAbsorbTables contract (tests/exact_coating.py), ray
by ray.

Every ray is a host ray; ray i draws from the stream SEED + i; every launch logs every event (record_every = 1,
max_events = 16, maxsteps = 64).  The anchors come first: on each case's twin WITHOUT absorptivity every judged surface
row is REFLECT iff u_k < R of `kernel_outcome`, for every ray and event -- that path is pinned to the referee
(tests/test_gpu_table_parity.py, tests/test_gpu_parity.py), so the anchors pin the restatement of R and the draw
positions independently of A.  Then every case: every judged surface row's kind equals `kernel_outcome`'s with the
uniform at the draw position the walk arrives at (family F: the first event from the world, draw 0; F-draw-or-not also
the ABSORB row behind the surface, whose `travelled` fixes with `==` whether the surface drew; I: from inside glass,
n = 1.5 -> 1, and the next events by the next draws; C: chains in a rotated box of up to 15 events (every row a history can hold), event k by draw k,
and eight rays launched alone, which the tail function finishes; L: the same judge on a tile of a node grid, under more
than 64 recorders, beside a mesh, and on the covered cells of a patterned coating on a rough node).  Every DETECT row
is the last of its history, carries the preceding row's direction bit for bit and the twin's row at the same index in
every other column; the rows before the first event whose outcome differs equal the twin's bit for bit.

Only the outcome and the draw position of an event are observable here: A is not logged.  The VALUE of A and of R is
held on the CPU (tests/test_coating_outcome_exact.py): bit for bit to the referee's table lookup and within the derived
bounds of the exact reference.  The conditions of every case (at least 100 rays of each outcome it is about, no
ambiguous ray, the threshold rays at exact equality, every named wrong rule caught by at least 20 rays) are asserted
there from the references alone.

Measured on an MI355X: every judged surface row of every case and of every twin equal to `kernel_outcome`, no exception
list.  Rows held per case (twin in brackets): F-scalar, F-on-R, F-on-sum, F-on-R-table, F-on-sum-table, F-one-row,
F-one-column, F-draw-or-not, I-matched, L-wide 1024 (1024); F-sweep 2048 (2048); F-both-tables 1605 (1982); F-clip 1024
(2025); I-tir 5709 (5709); I-near-critical 8019 (8130); C-chain 4986 (4986), of them 202 DETECT; L-tile 1617 (1959); L-mesh
1801 (2096); L-pattern 524 (524) covered points beside 500 holes; 519 ABSORB rows of F-draw-or-not at their draw
(docs/parity_chain.md, absorbing coatings)."""
import numpy as np
import pytest

from pvtrace_amd.engine import Session, native
from tests import exact_coating as X

pytestmark = pytest.mark.gpu

IDS = [c.name for c in X.CASES]
VALUES = ("position", "normal", "wavelength", "travelled", "duration", "hit", "container", "adjacent")


def trace(scene, pos, dirs, wl, launch=None, ray_offset=0):
    """The histories of one launch -> `History`.  `launch`: a dict that receives the launch's `launch_info()`."""
    n = len(pos)
    with Session(scene, emission="host") as session:
        result = session.collect(session.submit(n, X.SEED, host_rays=(pos, dirs, wl, ["r"] * n), record_every=1,
                                                max_events=X.ME, maxsteps=X.MAXSTEPS, ray_offset=ray_offset))
        data = {k: np.asarray(result.data[k]).copy() for k in X.History.COLUMNS}
        if launch is not None:
            launch.update(session.dscene.launch_info())
    return X.History(data, n)


_TRACED = {}


def traced(case, absorbing):
    """(inputs, history, launch info) of the case or of its twin, traced once."""
    key = (case.name, absorbing)
    if key not in _TRACED:
        x = X.inputs(case, absorbing=absorbing)
        launch = {}
        _TRACED[key] = (x, trace(x.scene, x.pos, x.dirs, x.wl, launch=launch), launch)
    return _TRACED[key]


# ---- the anchors: the twins without absorptivity ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_anchor_on_the_twin_every_surface_row_is_reflect_iff_u_is_below_r(case):
    x, hist, _ = traced(case, False)
    assert not x.compiled.has_absorbing_coatings and x.coat.absorb is None
    j = X.judge_history(x, hist, "kernel, no absorptivity")
    assert j.all_kinds[X.DETECT] == 0 and not np.any((hist.kind == X.DETECT) & live(hist))
    for e in j.events:
        assert (e.kind == X.REFLECT) == (e.kernel.draw and e.u < e.kernel.R), (case, e.ray, e.row, e.kind, e.u, e.kernel.R)
    print(f"kernel {case} twin: {len(j.events)} surface rows equal to kernel_outcome, {j.all_kinds}")
    assert len(j.events) >= (case.n if case.container != "pattern" else 300)
    if case.n_box != 1.0 and case.container != "pattern" and not case.coat.matched:
        assert len(j.events) >= case.n + 100          # (later events too: their draw positions)


def live(hist):
    return np.arange(hist.me)[None, :] < hist.counts[:, None]


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_the_kernel_outcome_agrees_with_the_contract_ray_by_ray(case):
    x, hist, launch = traced(case, True)
    twin_x, twin, _ = traced(case, False)
    # the path: every scene with an absorbing coating runs the extension family; the tile case is filed in a node grid,
    # the wide case has more than 64 recorders, the mesh case a mesh node
    assert x.compiled.has_absorbing_coatings and launch["variant"] == "rough", launch
    assert (native.node_grid_plan(x.compiled) is not None) == (case.container == "tile")
    if case.container == "tile":
        assert len(x.compiled.node_names) == 10
    assert (len(x.compiled.rec_node) > 64) == (case.container == "wide")
    assert bool(np.any(np.asarray(x.compiled.mesh_face_count) > 0)) == (case.container == "mesh")
    assert x.compiled.has_roughness == (case.container == "pattern")
    j = X.judge_history(x, hist, "kernel")            # every surface row's kind, the draw positions, the ABSORB rows
    print(f"kernel {case}: {len(j.events)} surface rows equal to kernel_outcome: {j.all_kinds}; first events {j.kinds}, drew "
          f"{j.drew}, did not {j.not_drew}; ABSORB rows held {len(j.absorb_rows)}; holes {j.holes}")
    counts = j.all_kinds if case.family == "C" else j.kinds
    for kind in case.needs:
        assert counts[kind] >= 100, (case, X.NAMES[kind], counts)
    if case.container != "pattern":
        assert sum(j.kinds.values()) == case.n
    else:
        assert sum(j.kinds.values()) >= 300 and j.holes >= 300
    if case.name == "F-draw-or-not":
        after = {k: sum(1 for _, at in j.absorb_rows if at == k) for k in (0, 1)}
        assert after[0] >= 100 and after[1] >= 100, (case, after)
    if case.name == "F-clip":
        assert j.kinds[X.TRANSMIT] == 0
    if case.name == "I-tir":
        assert j.kinds[X.REFLECT] == case.n and len(j.events) >= 2 * case.n - 50
    # every DETECT row: the twin's row at the same index, value for value; the preceding row's direction; the last row
    rows = live(hist)
    detect = (hist.kind == X.DETECT) & rows
    assert detect.sum() == j.all_kinds[X.DETECT] or case.container == "pattern", (case, detect.sum(), j.all_kinds)
    for i, row in zip(*np.nonzero(detect)):
        assert row == hist.counts[i] - 1 and row >= 1 and twin.counts[i] > row, (case, i, row)
        assert np.array_equal(hist.direction[i, row], hist.direction[i, row - 1]), (case, i, row, "direction")
        for key in VALUES:
            assert np.array_equal(getattr(hist, key)[i, row], getattr(twin, key)[i, row]), (case, i, row, key)
        assert twin.kind[i, row] == X.TRANSMIT, (case, i, row, "the twin transmits where the coating absorbs")
    if case.container == "pattern":
        assert detect.sum() >= 100
    # the rows up to the first event whose outcome differs are the twin's, bit for bit
    held = 0
    for i in range(case.n):
        m = min(int(hist.counts[i]), int(twin.counts[i]))
        differ = np.nonzero(hist.kind[i, :m] != twin.kind[i, :m])[0]
        if case.alpha:         # (behind the surface the absorber's tau* is one draw later where the surface drew)
            differ, m = differ[differ < 2], min(m, 2)
        m = int(differ[0]) if len(differ) else m
        for key in ("kind", "direction") + VALUES:
            assert np.array_equal(getattr(hist, key)[i, :m], getattr(twin, key)[i, :m]), (case, i, key)
        held += m
        if len(differ):
            assert hist.kind[i, m] == X.DETECT and twin.kind[i, m] == X.TRANSMIT, (case, i, m)
    assert held >= 2 * case.n - int(np.sum(hist.kind[:, 1] == X.DETECT)), (case, held)
    if case.name == "I-matched":
        first = hist.kind[:, 1] == X.TRANSMIT
        assert first.sum() >= 100 and np.array_equal(hist.direction[first, 1], hist.direction[first, 0])
    if case.family == "C":
        # eight rays with at least three reflections before their end, of both terminal kinds, each launched alone: the
        # tail function finishes a launch of one -- the same rows, held by the same reference
        lone = X.lone_rays(j)
        assert len(lone) == 8 and {j.ends[i] for i in lone} == {X.DETECT, X.TRANSMIT}, (case, lone)
        for i in lone:
            alone = trace(x.scene, x.pos[i:i + 1], x.dirs[i:i + 1], x.wl[i:i + 1], ray_offset=i)
            count = int(hist.counts[i])
            assert alone.counts[0] == count
            for key in ("kind", "direction") + VALUES:
                assert np.array_equal(getattr(alone, key)[0, :count], getattr(hist, key)[i, :count]), (case, i, key)
            ja = X.judge_history(X.subset(x, [i]), alone, "kernel, alone")
            assert ja.reflections.get(0, 0) >= 3 and ja.ends[0] == j.ends[i]
