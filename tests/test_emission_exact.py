"""The referee's emitter, the rule's float64 restatement and the host sampler against the exact reference of emission
and of the built-in phase turns (tests/exact_emission.py), ray by ray, on the CPU.

    oracle.emit (portable)  ==  kernel_emit           every ray, every component
    kernel_emit             within the exact rule's bound; no ray set aside
    emit._sample_light      within the bound of ITS operations, the same draws in the same order

Measured (worst |value - exact| / bound per family; docs/parity_chain.md, device emission):
    restatement = referee   directions 0.000  positions 0.830  hg 0.312  spectra 0.989  streams 0.840
    host sampler            directions 0.000  positions 0.797  hg 0.703  spectra 0.989  streams 0.840
(the wavelength bound, five roundings of the step and one of the sum, is sharp).  Without the clamp -- scratch copies
on the CPU -- the referee and the host sampler return NaN for 14 of the 2^20 rays of the hunt, the host sampler for 300
of the 600 planted grid draws, `material.henyey_greenstein` at each of its four; the seven wrong rules of
`exact_emission.FAULTS`, planted in such copies, each fail the case named in FAULT_CASES.
"""
import math

import mpmath
import numpy as np
import pytest

from fractions import Fraction as F

from oracle import oracle as O
from pvtrace_amd import material
from pvtrace_amd.engine import emit as host
from tests import exact_emission as X

CASES = X.CASES
IDS = [c.name for c in CASES]
WORST = {}


def _bundle(case):
    if not hasattr(case, "_kernel"):
        case._kernel = X.kernel_bundle(case.tables, case.n, case.emit_seed, case.ray_offset)
    return case._kernel


def test_the_stream_is_the_referees_on_64_keys_the_wrap_included():
    keys = [0, 1, 2, 77, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3, 2 ** 63, 2 ** 64 - 1, X.SALT, X.emit_key(2 ** 64 - 100, 99),
            X.emit_key(2 ** 64 - 100, 100), X.emit_key(2 ** 64 - 100, 101), X.trace_key(2 ** 64 - 5, 3, 9)]
    rng = np.random.default_rng(1)
    keys += [int(v) for v in rng.integers(0, 2 ** 63, 64 - len(keys))]
    assert len(keys) == 64 and X.emit_key(2 ** 64 - 100, 100) == X.SALT
    for key in keys:
        assert X.stream(key, 12) == O.uniforms(key, 12).tolist(), key
    assert X.stream(2 ** 64 + 5, 3) == X.stream(5, 3)


def test_the_array_forms_used_by_the_hunts_equal_the_scalar_ones():
    for emit_seed, offset in ((5, 0), (2 ** 64 - 100, 0), (77, 2 ** 40 + 3)):
        keys = X.emit_keys(emit_seed, offset, 300)
        assert [int(k) for k in keys] == [X.emit_key(emit_seed, offset + i) for i in range(300)]
        draws = X.stream_array(keys, 5)
        assert draws.tolist() == [X.stream(int(k), 5) for k in keys]
    for g in (0.9, -0.6, 1e-11, -1e-11, 3e-13):
        u = X.stream_array(X.emit_keys(9, 0, 400), 2)
        u[:3, 0] = X.EDGE_DRAWS
        d, raw = X.hg_turns(g, u[:, 0], u[:, 1])
        for i in range(400):
            want, info = X.kernel_turn(X.DIR_HG, g, (u[i, 0], u[i, 1]))
            assert tuple(d[i]) == want and raw[i] == info["raw"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_referee_equals_the_restatement_ray_for_ray(case):
    pos, dirs, wl, _, _ = _bundle(case)
    opos, odirs, owl = O.emit(case.tables, case.n, case.emit_seed, ray_offset=case.ray_offset, math_mode=O.MATH_PORTABLE)
    assert np.array_equal(owl, wl)
    assert np.array_equal(opos, pos)
    assert np.array_equal(odirs, dirs)          # (NaN would not compare equal: none is allowed)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_restatement_lies_within_the_exact_rules_bound(case):
    pos, dirs, wl, draws, infos = _bundle(case)
    refs = X.exact_bundle(case)
    assert len(refs) == case.n                                        # nothing is set aside
    assert np.array_equal(draws, [r["draws"] for r in refs])
    assert [i.get("branch", "z") for i in infos] == [r["branch"] for r in refs]
    ratio = X.worst_ratio(refs, pos, dirs, wl)
    WORST[case.name] = ratio
    print(f"{case.name}: worst |restatement - exact| / bound = {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_cases_reach_what_they_name(case):
    """From the reference alone."""
    refs = X.exact_bundle(case)
    n = case.n
    taken = {}
    for r in refs:
        for key in (r["branch"], r["wl_branch"]):
            taken[key] = taken.get(key, 0) + 1
    for branch in case.branches:
        assert taken.get(branch, 0) * 20 >= n, (branch, taken)
    if case.tied:
        assert sum(r["tie"] for r in refs) >= 50
    if case.small_table:
        segments = {r["segment"] for r in refs}
        x, cdf = case.tables.spectrum(0)
        if int(case.tables.wl_type[0]) == X.WL_SPECTRUM_HIST:
            want = {k for k in range(len(cdf)) if (cdf[k] > (cdf[k - 1] if k else 0.0)) or (k == len(cdf) - 1 and cdf[k] < 1.0)}
        else:
            want = {k for k in range(len(cdf) - 1) if cdf[k + 1] > cdf[k]}
        assert want <= segments, (want, segments)
    if case.signs:
        d = np.array([[float(v) for v in r["dir"]] for r in refs])
        assert np.all((d > 0).any(axis=0)) and np.all((d < 0).any(axis=0))
    if case.name == "R-seven-lights":
        assert case.ray_offset % 7 != 0 and {r["light"] for r in refs} == set(range(7))
    if case.name == "R-seed-wraps":
        assert case.emit_seed + case.ray_offset < 2 ** 64 <= case.emit_seed + case.ray_offset + case.n - 1


def _host_tables(case):
    """The tables as the host's classifier writes them: |g| < 1e-12 is the isotropic delegate (classify_direction)."""
    g = case.tables.dir_param[case.tables.dir_type == X.DIR_HG]
    return None if np.any(np.abs(g) < 1e-12) else case.tables


def _host_light(tab, li, draws):
    """`_sample_light` of light li fed column k of `draws` (rays x 8) at its k-th uniform(n) call -> (pos, dir, wl, calls)."""
    calls = []

    def uniform(n):
        assert n == len(draws)
        calls.append(len(calls))
        return draws[:, calls[-1]].copy()

    pos, direc, wl = host._sample_light(tab, li, len(draws), uniform)
    return pos, direc, wl, len(calls)


@pytest.mark.parametrize("case", [c for c in CASES if _host_tables(c) is not None],
                         ids=[c.name for c in CASES if _host_tables(c) is not None])
def test_the_host_sampler_takes_the_same_draws_and_lies_within_its_bound(case):
    tab = case.tables
    refs = X.exact_bundle(case)
    worst = 0.0
    for li in range(tab.n_lights):
        rows = [i for i in range(case.n) if refs[i]["light"] == li]
        draws = np.array([X.stream(X.emit_key(case.emit_seed, case.ray_offset + i), 8) for i in rows])
        pos, direc, wl, calls = _host_light(tab, li, draws)
        assert all(refs[i]["draws"] == calls for i in rows)            # the same number of draws, column k at call k
        pt, pp = int(tab.pos_type[li]), [float(v) for v in tab.pos_param[li]]
        dt, prm = int(tab.dir_type[li]), float(tab.dir_param[li])
        with mpmath.workdps(X.DIGITS):
            for j, i in enumerate(rows):
                ref = refs[i]
                pairs = [(wl[j], X._mp(ref["wl"]), ref["e_wl"])]
                if pt != X.POS_POINT:
                    _, bp, _ = X.exact_position(pt, pp, ref["pos_draws"], ulps=X.H_ULP)
                    pairs += [(pos[j, a], ref["local_pos"][a], bp[a].e + X.SLACK) for a in range(3)]
                else:
                    assert not pos[j].any()
                if dt != X.DIR_Z:
                    bound = X.host_turn_bound(dt, prm, ref["dir_draws"])
                    pairs += [(direc[j, a], ref["local_dir"][a], bound[a]) for a in range(3)]
                else:
                    assert tuple(direc[j]) == (0.0, 0.0, 1.0)
                for got, want, bound in pairs:
                    assert math.isfinite(got)
                    err = abs(float(X._mp(F(float(got))) - want))
                    if err > 0.0:
                        worst = max(worst, err / bound if bound > 0.0 else math.inf)
    print(f"{case.name}: worst |host - exact| / bound = {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ planted draws
def _judge_turn(kind, param, u, host_too=True):
    """One planted turn: the restatement, the referee and (where it has the delegate) the host sampler are finite, of unit
    length within the bound, and within the bound of the exact value."""
    got, info = X.kernel_turn(kind, param, u)
    exact, bound, branch = X.exact_turn(kind, param, u)
    assert info["branch"] == branch
    results = [("restatement", got, bound)]
    if host_too:
        tab = X.Tables([dict(dir=(kind, param))])
        _, direc, _, calls = _host_light(tab, 0, np.array([list(u) + [0.0] * 6]))
        assert calls == 2
        results.append(("host", tuple(direc[0]), X.host_turn_bound(kind, param, u)))
    with mpmath.workdps(X.DIGITS):
        for who, d, e in results:
            assert all(math.isfinite(v) for v in d), (who, kind, param, u, d)
            norm2 = sum(F(float(v)) ** 2 for v in d)
            # |d|^2 - 1 = 2 d . (d - exact) + |d - exact|^2 for a unit exact direction
            slack = 2.0 * sum(abs(float(x)) * b for x, b in zip(exact, e)) + sum(b * b for b in e)
            assert abs(float(norm2 - 1)) <= slack, (who, kind, param, u)
            for a in range(3):
                assert abs(float(X._mp(F(float(d[a]))) - exact[a])) <= e[a], (who, kind, param, u, a)


def test_planted_draws_at_the_ends_of_the_grid_for_200_asymmetries():
    grid = X.hg_grid()
    assert len(grid) == 200 and min(abs(g) for g in grid) == 1e-12 and max(grid) == 0.999
    clamped = 0
    for g in grid:
        for u0 in X.EDGE_DRAWS:
            _judge_turn(X.DIR_HG, g, (u0, 0.3125))
            raw = X.kernel_turn(X.DIR_HG, g, (u0, 0.3125))[1]["raw"]
            clamped += abs(raw) > 1.0
            # the referee's single-turn hook draws from a stream; its rule is pinned by the bundle cases above
    assert clamped >= 20          # the planted draws do reach the clamp
    for u0 in X.EDGE_DRAWS:       # the cases of the issue's table
        for g in (0.3, 0.85, 0.99, 0.1, 1e-10, 1e-11, -1e-11):
            _judge_turn(X.DIR_HG, g, (u0, 0.75))
    assert X.kernel_turn(X.DIR_HG, 0.3, (0.0, 0.0))[1]["raw"] < -1.0


def test_planted_draws_of_the_disc_the_lambertian_and_the_isotropic_branch():
    top = 1.0 - 2.0 ** -53
    for u in ((top, 0.4), (top, top), (0.0, 0.0), (2.0 ** -53, top)):
        _judge_turn(X.DIR_LAMBERTIAN, 0.0, u)
        _judge_turn(X.DIR_CONE, 0.5, u)
        _judge_turn(X.DIR_CONE, math.pi / 2, u)
    for g1 in (0.0, 0.25, top):
        for g2 in (0.0, 2.0 ** -53, 0.5, top):    # g2 = 0: straight down, the sine exactly zero
            _judge_turn(X.DIR_ISOTROPIC, 0.0, (g1, g2))
    assert X.kernel_turn(X.DIR_ISOTROPIC, 0.0, (0.25, 0.0))[0] == (0.0, 0.0, -1.0)
    # the disc at the last draw of the grid: the restatement and the host within the exact position's bound
    for u in ((top, top), (0.0, top), (top, 0.0), (0.625, top)):
        tab = X.Tables([dict(pos=(X.POS_CIRCLE, (2.5, 0.0, 0.0)))])
        lp, bp, k = X.exact_position(X.POS_CIRCLE, [2.5, 0.0, 0.0], list(u))
        _, hb, _ = X.exact_position(X.POS_CIRCLE, [2.5, 0.0, 0.0], list(u), ulps=X.H_ULP)
        pos, _, _, calls = _host_light(tab, 0, np.array([list(u) + [0.0] * 6]))
        assert k == 2 and calls == 2
        ang = X.TWO_PI_D * u[0]
        rad = math.sqrt(u[1]) * 2.5
        mine = (rad * X._p("cos", ang), rad * X._p("sin", ang))
        with mpmath.workdps(X.DIGITS):
            for a in range(2):
                assert abs(float(X._mp(F(mine[a])) - lp[a])) <= bp[a].e + X.SLACK
                assert abs(float(X._mp(F(float(pos[0, a]))) - lp[a])) <= hb[a].e + X.SLACK


def test_the_referee_and_the_host_sampler_at_a_vanishing_asymmetry_over_a_million_rays():
    """Streams reach the clamp at |g| = 1e-11, about once in 10^5 draws: the referee in both modes and the host sampler
    give finite unit directions there (NaN before the clamp), the portable referee the clamped restatement's."""
    n, g, emit_seed = 2 ** 20, 1e-11, 2
    tab = X.Tables([dict(dir=(X.DIR_HG, g), pose=np.eye(4))])
    u = X.stream_array(X.emit_keys(emit_seed, 0, n), 2)
    want, raw = X.hg_turns(g, u[:, 0], u[:, 1])
    beyond = np.flatnonzero(np.abs(raw) > 1.0)
    print("rays of 2^20 whose cosine leaves [-1, 1] before the clamp:", len(beyond))
    assert len(beyond) >= 5
    _, dirs, _ = O.emit(tab, n, emit_seed, math_mode=O.MATH_PORTABLE)
    assert np.array_equal(dirs, want) and np.all(np.abs(dirs[beyond, 2]) == 1.0)
    _, libm, _ = O.emit(tab, n, emit_seed, math_mode=O.MATH_LIBM)
    _, direc, _, calls = _host_light(tab, 0, np.column_stack((u, np.zeros((n, 6)))))
    assert calls == 2
    for d in (libm, direc):
        assert np.all(np.isfinite(d)) and np.all(np.abs(d[beyond, 2]) == 1.0)
        # sin^2 + cos^2 of the two computed angles: each function within 2 H_ULP U, so each square within 4 H_ULP U;
        # st^2 (cp^2 + sp^2) + ct^2 is 1 within 8 H_ULP U and the six roundings of the products and sums
        assert np.max(np.abs((d * d).sum(axis=1) - 1.0)) <= (8.0 * X.H_ULP + 6.0) * X.U


def test_the_scalar_host_delegate_is_clamped_too(monkeypatch):
    """material.henyey_greenstein at the draws where its cosine leaves [-1, 1]: a finite unit vector."""
    for g, p in ((0.3, 0.0), (0.85, 0.0), (0.99, 0.0), (0.1, 1.0 - 2.0 ** -53)):
        feed = iter([p, 0.375])
        monkeypatch.setattr(material.np.random, "uniform", lambda *a, **k: next(feed))
        d = material.henyey_greenstein(g)
        assert all(math.isfinite(v) for v in d) and abs(sum(v * v for v in d) - 1.0) < 1e-15
        assert abs(d[2]) == 1.0


# ------------------------------------------------------------------------------------------------ the wrong rules
FAULT_CASES = {"bisect-lt": "S-tied-linear", "searchsorted-right": "S-tied-hist", "hg-draws-swapped": "H-0.9",
               "cone-draws-swapped": "P-rect-cone-0.5", "pose-transposed": "D-pose-only", "salt-dropped": "R-seven-lights",
               "gi-mod-2^32": "R-offset-2^40"}


@pytest.mark.parametrize("fault", X.FAULTS)
def test_each_wrong_rule_fails_a_named_case(fault):
    """From the references alone: the rule with the fault planted leaves the exact rule's bound on its case (and so a
    referee or a kernel with that fault, which must EQUAL the right restatement, fails there)."""
    case = X.BY_NAME[FAULT_CASES[fault]]
    pos, dirs, wl, _, _ = _bundle(case)
    bpos, bdirs, bwl, _, _ = X.kernel_bundle(case.tables, case.n, case.emit_seed, case.ray_offset, fault=fault)
    moved = (pos != bpos).any(axis=1) | (dirs != bdirs).any(axis=1) | (wl != bwl)
    assert moved.sum() >= 50, moved.sum()
    assert X.worst_ratio(X.exact_bundle(case), bpos, bdirs, bwl) > 1.0
