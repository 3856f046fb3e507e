"""Absorbing coatings without a GPU, exactly and per ray (tests/exact_coating.py): the float64 restatement of the
PvtCoatingAbsorbTables contract against the exact one within its derived bounds, its table values against the referee's
lookup bit for bit, the conditions of every case and the coverage of the named wrong rules from the references alone,
and the host rule (`Surface.outcome`, `CoatedSurfaceDelegate.reflectivity` / `.absorptivity`, `photon_tracer` on the
host objects) against the exact reference on the rays tests/test_gpu_coating_outcome_exact.py traces.

The chains the conditions are counted on are the REFEREE's histories of the twins without absorptivity: the twin shares
every draw with the case up to the first DETECT (a DETECT happens only where the twin transmits on the same draw), so
the case's chain is the twin's, cut where `kernel_outcome` says DETECT.  Nothing but the outcome and the draw position
of an event carries over to the GPU -- A is not logged -- so the value-level checks are the ones here.

Measured on these cases (worst |value - exact| / bound over every judged event; 0 where the value is a scalar or an
exact 0 and equality is asked instead).  `kernel_outcome`, R then A: F-on-R-table 0.775, 0; F-on-sum-table 0, 0.497;
F-sweep 0, 0.298; F-one-row 0, 0.777; F-one-column 0, 0.301; F-both-tables 0.369, 0.401; F-clip 0.045, 0 (Fresnel);
F-draw-or-not 0, 0.587; I-tir 0.039, 0; I-matched 0, 0.182; I-near-critical 0.108, 0 (Fresnel, its later events);
C-chain 0.035, 0.332; L-tile 0.352, 0.349; L-wide 0, 0.276; L-mesh 0.049, 0.578; L-pattern 0, 0.224; F-scalar, F-on-R and
F-on-sum 0, 0.  The host rule (`CoatedSurfaceDelegate.reflectivity`, `.absorptivity`; first events of F and I), R then A:
F-on-R-table 0.775, 0; F-on-sum-table 0, 0.497; F-sweep 0, 0.393; F-one-row 0, 0.777; F-one-column 0, 0.330; F-both-tables
0.385, 0.427; F-clip 0.036, 0; F-draw-or-not 0, 0.587; I-matched 0, 0.351; the scalar cases 0, 0.  No event of any case is
ambiguous under either bound; the rays constructed onto a threshold sit at exact equality (1 ray in F-on-R and F-on-sum,
193 in F-on-R-table, 74 in F-on-sum-table).  Wrong rules, rays whose reference changes: le-R 193 (F-on-R-table), le-sum 74
(F-on-sum-table), transposed 422, no-clamp-wl-lo 95, no-clamp-wl-hi 121, no-clamp-angle-lo 133, no-clamp-angle-hi 82,
no-draw-at-R0 2048 (F-sweep), swapped 663 and draw-at-A0 361 (F-draw-or-not), refracted 415 (I-matched), degrees 445
(F-one-column), absorb-under-tir 1024 (I-tir), clip-sum 74 (F-clip)."""
import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd import Event, Ray
from pvtrace_amd.algorithm import photon_tracer
from pvtrace_amd.material import ReflectivityTable
from tests import exact_coating as X

IDS = [c.name for c in X.CASES]
HOST_KIND = {Event.REFLECT: X.REFLECT, Event.TRANSMIT: X.TRANSMIT, Event.DETECT: X.DETECT}


class Feeding:
    """`np.random.uniform` hands out `draws` in order while the block runs (a list; it is emptied)."""

    def __init__(self, draws):
        self.draws = draws

    def __enter__(self):
        self.saved = np.random.uniform
        np.random.uniform = lambda low=0.0, high=1.0, size=None: low + (high - low) * self.draws.pop(0)

    def __exit__(self, *exc):
        np.random.uniform = self.saved


def referee_history(x):
    data = O.trace_bundle(x.compiled, x.pos, x.dirs, x.wl, X.SEED, X.MAXSTEPS, X.ME, 0, 4, 1, math_mode=O.MATH_PORTABLE)
    return X.History(data, x.case.n)


def first_rows(x):
    """The first surface row of rays sent onto the top face from above, written down from the geometry: for the one
    scene the referee does not trace (a rough node with a patterned coating)."""
    n = x.case.n
    data = {k: np.zeros((n, X.ME) + ((3,) if k in X.History.VECTORS else ())) for k in X.History.COLUMNS if k != "counts"}
    data = {k: v.astype(np.int64) if k in X.History.INTS else v for k, v in data.items()}
    data["counts"] = np.full(n, 2)
    t = (1.0 - x.pos[:, 2]) / x.dirs[:, 2]
    data["position"][:, 0], data["direction"][:, 0], data["wavelength"][:, 0] = x.pos, x.dirs, x.wl
    data["position"][:, 1] = x.pos + x.dirs * t[:, None]
    data["position"][:, 1, 2] = 1.0
    data["normal"][:, 1] = X.TOP
    data["kind"][:, 1], data["hit"][:, 1], data["adjacent"][:, 1] = X.TRANSMIT, x.node_id, x.node_id
    return X.History(data, n)


_CHAINS = {}


def chains(case):
    """`judge_history` of the case on the referee's twin history, once."""
    if case.name not in _CHAINS:
        x = X.inputs(case)
        if case.container == "pattern":
            j = _first_only(x, first_rows(x))
        else:
            twin = X.inputs(case, absorbing=False)
            assert np.array_equal(twin.pos, x.pos) and np.array_equal(twin.dirs, x.dirs) and np.array_equal(twin.wl, x.wl)
            j = X.judge_history(x, referee_history(twin), "referee", own=False)
        _CHAINS[case.name] = j
    return _CHAINS[case.name]


def _first_only(x, hist):
    """The first events of a synthetic history: what `judge_history` does with own=False, without a twin's kinds."""
    out = X.Judged()
    out.events, out.absorb_rows, out.ends, out.reflections, out.holes = [], [], {}, {}, 0
    out.kinds = {k: 0 for k in X.SURFACE}
    out.drew = out.not_drew = 0
    for i in range(hist.n):
        coat = X.covering(x, hist, i, 1)
        if coat is None:
            out.holes += 1
            continue
        e = X.Event()
        e.ray, e.row, e.at = i, 1, 0
        e.normal, e.d_in, e.wl = hist.normal[i, 1].copy(), hist.direction[i, 0].copy(), float(hist.wavelength[i, 0])
        e.n1, e.n2, e.coat, e.u = 1.0, x.index[x.node_id], coat, float(x.draws[i, 0])
        e.kernel = e.outcome()
        e.kind = e.kernel.kind
        out.events.append(e)
        out.kinds[e.kernel.kind] += 1
        out.drew += e.kernel.draw
        out.ends[i] = e.kernel.kind
    out.all_kinds = dict(out.kinds)
    return out


def table_value(table, wl, theta):
    return O.coat_table_r(table.wavelength, table._angle_axis, table._grid, wl, theta)


def ratio(got, want, bound):
    """|got - want| / bound; equality is asked where the bound is 0."""
    with X.precise:
        err = abs(X.mpf(got) - want)
        if bound == 0:
            assert err == 0, (got, float(want))
            return 0.0
        return float(err / bound)


# ---- the restatements on events worked by hand -----------------------------------------------------------------------------
def test_the_restatement_on_events_worked_by_hand():
    up, down = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
    k = X.kernel_outcome(up, down, 555.0, 1.0, 1.5, None, 0.03)
    assert k.c1 == 1.0 and k.theta == 0.0 and abs(k.R - 0.04) < 1e-15 and k.kind == X.REFLECT and k.draw
    k = X.kernel_outcome(up, down, 555.0, 1.0, 1.5, X.Coat(0.25, 0.5), 0.25)
    assert (k.kind, k.draw, k.R, k.A) == (X.DETECT, True, 0.25, 0.5)                 # u = R is not reflected
    assert X.kernel_outcome(up, down, 555.0, 1.0, 1.5, X.Coat(0.25, 0.5), 0.75).kind == X.TRANSMIT   # u = R + A is not absorbed
    assert X.kernel_outcome(up, down, 555.0, 1.0, 1.5, X.Coat(0.25, 0.5), 0.7499).kind == X.DETECT
    k = X.kernel_outcome(up, down, 555.0, 1.0, 1.5, X.Coat(0.0, 0.0, matched=True), 0.0)
    assert (k.kind, k.draw) == (X.TRANSMIT, False)                                     # R = 0 and A = 0: no draw
    k = X.kernel_outcome(up, down, 555.0, 1.0, 1.5, X.Coat(0.0, 0.5, matched=True), 0.4)
    assert (k.kind, k.draw) == (X.DETECT, True)                                        # R = 0, A > 0: the draw is taken
    d = (0.8, 0.0, 0.6)                                                                # beyond the critical angle of 1.5 -> 1
    k = X.kernel_outcome(up, d, 555.0, 1.5, 1.0, X.Coat(None, 1.0), 0.999)
    assert (k.kind, k.draw, k.R, k.tir) == (X.REFLECT, True, 1.0, True)
    k = X.kernel_outcome(up, d, 555.0, 1.5, 1.0, X.Coat(0.0, 1.0, matched=True), 0.999)
    assert (k.kind, k.R, k.A) == (X.DETECT, 0.0, 1.0)
    table = X.AbsorptivityTable([400.0, 800.0], [[0.0, 0.2], [0.6, 1.0]], angle=[0.0, 90.0])
    assert X.kernel_lookup(table, 600.0, 0.0) == 0.1 and X.kernel_lookup(table, 800.0, 2.0) == 1.0
    assert X.kernel_lookup(table, 400.0, 45.0 * X.RAD_PER_DEG) == 0.3
    with X.precise:
        e = X.exact_outcome(up, down, 555.0, 1.0, 1.5, X.Coat(None, table), 0.5)
        assert abs(e.R - X.mpf("0.04")) < 1e-30 and e.A == X.to_mpf(X.F(155, 400) * X.fr(0.2)) and e.kind == X.TRANSMIT


# ---- the cases: cross-checks and conditions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_the_conditions_hold_and_the_restatement_lies_within_the_exact_bounds(case):
    x = X.inputs(case)
    j = chains(case)
    worst_r = worst_a = 0.0
    ambiguous = 0
    on = set(x.on_threshold)
    for e in j.events:
        k = e.kernel
        coat = e.coat
        if coat is not None and isinstance(coat.absorb, ReflectivityTable):
            assert k.A == table_value(coat.absorb, e.wl, k.theta), (case, e.ray, e.row, "A", k.A)
        if coat is not None and isinstance(coat.refl, ReflectivityTable) and not (k.tir and not coat.matched):
            assert k.R == table_value(coat.refl, e.wl, k.theta), (case, e.ray, e.row, "R", k.R)
        r = e.exact()
        ambiguous += r.ambiguous
        worst_r = max(worst_r, ratio(k.R, r.R, r.e_R))
        worst_a = max(worst_a, ratio(k.A, r.A, r.e_A))
        assert worst_r <= 1.0 and worst_a <= 1.0, (case, e.ray, e.row, k.R, float(r.R), k.A, float(r.A), worst_r, worst_a)
        if not r.ambiguous:
            assert (k.kind, k.draw, k.tir) == (r.kind, r.draw, r.tir), (case, e.ray, e.row, k.kind, r.kind, k.draw, r.draw)
        if e.ray in on and e.row == 1:
            # the constructed rays: exact equality, where the bounds are 0 and the contract's "<" decides
            assert not r.ambiguous and r.e_R == 0 and r.e_sum == 0, (case, e.ray)
            if "on-R" in case.name:
                assert e.u == k.R and k.kind == r.kind == X.DETECT, (case, e.ray, e.u, k.R, k.kind)
            else:
                assert float(np.float64(k.R) + np.float64(k.A)) == e.u and k.kind == r.kind == X.TRANSMIT, (case, e.ray, e.u, k.R, k.A)
    print(f"{case}: {len(j.events)} events; first events {j.kinds}; drew {j.drew}, did not {j.not_drew}; worst |R - exact| / e_R "
          f"{worst_r:.3f}, |A - exact| / e_A {worst_a:.3f}; ambiguous {ambiguous}")
    assert ambiguous == 0, (case, ambiguous)
    counts = j.all_kinds if case.family == "C" else j.kinds
    for kind in case.needs:
        assert counts[kind] >= 100, (case, X.NAMES[kind], counts)
    first = [e for e in j.events if e.row == 1]
    if case.container != "pattern":
        assert len(first) == case.n and all(e.coat is not None for e in first), (case, len(first))
    else:
        assert len(first) >= 300 and j.holes >= 300, (case, len(first), j.holes)
    if on or case.name.startswith("F-on-"):
        assert len(on) >= (1 if not case.name.endswith("-table") else 50), (case, len(on))
    if case.name == "F-clip":
        assert j.kinds[X.TRANSMIT] == 0 and all(e.kernel.R + e.kernel.A > 1.0 for e in first), case
    if case.name == "F-draw-or-not":
        assert j.not_drew >= 100 and j.drew >= 100, (case, j.drew, j.not_drew)
        knot = [e for e in first if e.wl == 500.0]
        assert knot and all(not e.kernel.draw and e.kernel.A == 0.0 for e in knot)
        assert any(e.kernel.draw for e in first if 500.0 < e.wl < 500.0001)          # one ulp beyond the knot
        assert all(e.kernel.draw == (e.wl > 500.0) for e in first)
    if case.name == "I-tir":
        assert all(e.kernel.tir and e.kernel.draw and e.kernel.kind == X.REFLECT for e in first)
        assert sum(len([e for e in j.events if e.ray == i]) >= 2 for i in range(0, case.n, 16)) >= 32   # draw 1 decides the next
    if case.name == "I-matched":
        assert all(e.kernel.tir and e.kernel.R == 0.0 for e in first)
    if case.name == "I-near-critical":
        tir = sum(e.kernel.tir for e in first)
        assert tir >= 100 and len(first) - tir >= 100, (case, tir)
        assert all(abs(e.kernel.theta - X.CRIT) <= 1.0001e-7 for e in first)
    if case.name in ("F-sweep", "F-both-tables"):
        for table in (t for t in (x.coat.refl, x.coat.absorb) if isinstance(t, ReflectivityTable)):
            for w in table.wavelength:
                assert any(e.wl == w for e in first), (case, "no ray on the wavelength knot", w)
            for deg in table._angle_axis:
                knot = float(np.float64(deg) * np.float64(X.RAD_PER_DEG))
                near = [e.kernel.theta - knot for e in first if abs(e.kernel.theta - knot) <= 1.0001e-9]
                assert any(v < 0 for v in near) and any(v > 0 for v in near), (case, "no rays either side of the angle knot", deg)
            assert min(e.wl for e in first) < table.wavelength[0] - 20.0 and max(e.wl for e in first) > table.wavelength[-1] + 20.0
    if case.family == "C":
        lone = X.lone_rays(j)
        assert len(lone) == 8 and {j.ends[i] for i in lone} == {X.DETECT, X.TRANSMIT}, (case, lone)


def test_every_wrong_rule_changes_the_reference_for_twenty_rays_of_a_case():
    caught = {}
    for fault in X.FAULTS:
        best = max(((len(X.faulted_rays(chains(case).events, fault)), case.name) for case in X.CASES))
        caught[fault] = best
        print(f"{fault}: {best[0]} rays of {best[1]}")
    assert all(n >= 20 for n, _ in caught.values()), caught


# ---- the host rule -----------------------------------------------------------------------------------------------------------
HOSTED = [c for c in X.CASES if c.family in ("F", "I")]


@pytest.mark.parametrize("case", HOSTED, ids=[c.name for c in HOSTED])
def test_the_host_rule_agrees_with_the_exact_reference_ray_by_ray(case):
    x = X.inputs(case)
    world = x.scene.root
    box = x.box
    skin = box.geometry.material.surface
    above = case.rays == "above"
    container, adjacent = (world, box) if above else (box, world)
    worst_r = worst_a = 0.0
    ambiguous = detected = 0
    for i in range(case.n):
        draws = [float(v) for v in x.draws[i, :8]]
        with Feeding(draws):
            hist = list(photon_tracer.step_forward(x.scene, Ray(tuple(x.pos[i]), tuple(x.dirs[i]), float(x.wl[i])), maxsteps=1,
                                                   backend="host"))
        ray, event, meta = hist[1]
        r = X.exact_outcome(X.TOP, x.dirs[i], x.wl[i], x.index[0] if above else case.n_box, case.n_box if above else x.index[0],
                            x.coat, x.draws[i, 0], who="host")
        ambiguous += r.ambiguous
        if not r.ambiguous:
            assert HOST_KIND[event] == r.kind, (case, i, event, r.kind, float(r.R), float(r.A), x.draws[i, 0])
            assert 8 - len(draws) == int(r.draw), (case, i, "draws taken", 8 - len(draws), r.draw)
        else:
            assert HOST_KIND[event] in r.kinds, (case, i, event)
        t = (1.0 - x.pos[i, 2]) / x.dirs[i, 2]
        point = x.pos[i] + t * x.dirs[i]
        at = Ray(tuple(point), tuple(x.dirs[i]), float(x.wl[i]))
        worst_r = max(worst_r, ratio(float(skin.delegate.reflectivity(skin, at, box.geometry, container, adjacent)), r.R, r.e_R))
        worst_a = max(worst_a, ratio(float(skin.delegate.absorptivity(skin, at, box.geometry, container, adjacent)), r.A, r.e_A))
        assert worst_r <= 1.0 and worst_a <= 1.0, (case, i, worst_r, worst_a)
        if event == Event.DETECT:
            # the DETECT row of the kernel rule: the hit point, the INCOMING direction, the wavelength, the ids of a
            # REFLECT or TRANSMIT row there; and the last row
            detected += 1
            assert len(hist) == 2
            assert np.allclose(ray.position, point, rtol=0.0, atol=1e-12) and abs(ray.position[2] - 1.0) <= 1e-12
            assert tuple(ray.direction) == tuple(x.dirs[i]) and ray.wavelength == x.wl[i]
            assert (meta["hit"], meta["container"], meta["adjacent"]) == ("box", container.name, adjacent.name)
            assert tuple(meta["normal"]) == X.TOP
    print(f"{case}: host worst |R - exact| / e_R {worst_r:.3f}, |A - exact| / e_A {worst_a:.3f}; DETECT {detected}; ambiguous {ambiguous}")
    assert ambiguous == 0
    if X.DETECT in case.needs:
        assert detected >= 100
