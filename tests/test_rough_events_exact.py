"""The host's rough-surface sampler (`ggx_visible_normal`, `rough_fresnel_reflectivity`, `rough_directions`,
pvtrace_amd/material.py) against the exact reference of the PvtSurfaceTables contract (tests/exact_events.py), one event
at a time, on every case of both families: generic rays on a box, a rotated box, a sphere, a cylinder, a mesh and a
tile of a node grid, and the edge rays (exact normal incidence, signed zeros, grazing incidence, the critical angle,
rays inside a coordinate plane).  The same cases, rays and draws hold the kernel in
tests/test_gpu_rough_events_exact.py; here the reference, its margins, the share of ambiguous rays and the conditions of
`check_rough_conditions` are proven without a GPU.  The geometric normal is the host geometry's at the host's own
crossing (the kernel test reads the logged one); the host takes cos and sin of fl(2 pi u_b) from numpy, so its bound
carries TRIG_HOST where the kernel's carries TRIG_KERNEL.

Measured on these cases (worst |direction - exact| / bound): 0.079 in the generic family, 0.085 in the edge family (the
critical angle at alpha = 1e-4); no ray of any case is ambiguous."""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

from oracle import oracle as O
from pvtrace_amd.engine import compile_scene
from pvtrace_amd.material import ggx_visible_normal, rough_directions, rough_fresnel_reflectivity
from tests import exact_events as X

SEED = X.SEED


def case_inputs(case, alpha=None):
    """(scene, block, compiled, node id, positions, directions, wavelengths, inside, n1, n2, draws) of a case: the
    draws are the first three uniforms of each ray's stream `SEED + index`, as the kernel draws u_a, u_b and u."""
    scene, block = case.scene(alpha)
    compiled = compile_scene(scene)
    node_id = list(compiled.node_names).index(block.name)
    pos, dirs, wl, inside = case.world_rays(compiled, node_id)
    n1, n2 = case.indices(wl, inside)
    draws = np.array([O.uniforms(SEED + i, 3) for i in range(case.n)])
    return scene, block, compiled, node_id, pos, dirs, wl, inside, n1, n2, draws


def host_normals(case, block, compiled, node_id, pos, dirs):
    """The geometric normal (outward, world frame) at the first crossing of every ray with the node, by the host's own
    geometry."""
    M = np.asarray(compiled.local_to_world[node_id], dtype=np.float64)
    W = np.asarray(compiled.world_to_local[node_id], dtype=np.float64)
    out = np.zeros((case.n, 3))
    for i in range(case.n):
        o = W[:3, :3] @ pos[i] + W[:3, 3]
        v = W[:3, :3] @ dirs[i]
        points = block.geometry.intersections(tuple(o), tuple(v))
        assert points, (case, i)
        nearest = min(points, key=lambda p: float(np.dot(np.subtract(p, o), v)))
        out[i] = M[:3, :3] @ np.asarray(block.geometry.normal(nearest), dtype=np.float64)
    return out


def host_events(case, dirs, normals, n1, n2, draws):
    """The host's (reflect, direction, m, R) of every ray.  Under test are the three functions the host delegate is
    made of -- m, R and the two directions.  The decision `R > 0 and u < R` is written HERE, from item 4: on the host it
    is taken by the tracer's surface step from numpy's global generator (`FresnelSurfaceDelegate.reflectivity`, then the
    step's own draw), which has no stream to replay, so neither the host's decision nor its draw order is held by this
    file; the kernel's are, in tests/test_gpu_rough_events_exact.py."""
    out = []
    for i in range(case.n):
        m = ggx_visible_normal(normals[i], dirs[i], case.alpha, draws[i, 0], draws[i, 1])
        R = rough_fresnel_reflectivity(-float(np.dot(dirs[i], m)), float(n1[i]), float(n2[i]))
        reflected, transmitted = rough_directions(dirs[i], normals[i], m, float(n1[i]), float(n2[i]))
        reflect = bool(R > 0.0 and draws[i, 2] < R)
        assert reflect or transmitted is not None, (case, i)
        out.append((reflect, reflected if reflect else transmitted, m, R))
    return out


def test_the_reference_on_events_worked_by_hand():
    with mp.workdps(X.DIGITS):
        n1, n2 = 1.0, 1.5
        # normal incidence, u_a = 0: Vh = (0, 0, 1), s = 1, t1 = t2 = 0, Nh = Vh: m = N exactly, whatever alpha and u_b
        for N in ((0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, -1.0, -0.0)):
            d = tuple(-c for c in N)
            r = X.exact_rough_event(d, N, 0.4, n1, n2, 0.0, 0.37, 0.5)
            assert r.fallback and [float(c) for c in r.m] == [float(c) for c in N]
            assert abs(r.R - mpf(1) / 25) < 1e-50                       # ((n1 - n2) / (n1 + n2))^2
            assert not r.reflect and max(abs(r.transmitted[c] - mpf(d[c])) for c in range(3)) < 1e-50
            assert X.exact_rough_event(d, N, 0.4, n1, n2, 0.0, 0.37, 0.03).reflect
        # normal incidence, alpha -> 0: m -> N, whatever the draws (|m - N| of the order of alpha)
        r = X.exact_rough_event((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), 1e-9, n1, n2, 0.83, 0.21, 0.5)
        assert max(abs(r.m[c] - mpf((0.0, 0.0, 1.0)[c])) for c in range(3)) < 1e-8 and r.m[2] < 1
        # normal incidence on +z, the fallback frame T1 = (1, 0, 0), T2 = (0, 1, 0): u_b = 0 puts Nh in the xz-plane,
        # Nh = (r, 0, sqrt(1 - r^2)) with r = sqrt(u_a), and m = normalize(alpha r, 0, sqrt(1 - r^2))
        r = X.exact_rough_event((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), 0.5, n1, n2, 0.25, 0.0, 0.5)
        L = math.sqrt(0.0625 + 0.75)
        assert abs(r.m[0] - mpf(0.25) / mpf(0.8125).sqrt()) < 1e-50 and r.m[1] == 0 and abs(float(r.m[2]) - math.sqrt(0.75) / L) < 1e-15
        # u_a = 0 at oblique incidence in the xz-plane about +z, alpha = 1 (Vh = v): t1 = 0, t2 = 1 - s = (1 - Vh.z) / 2, so
        # Nh = t2 T2 + sqrt(1 - t2^2) Vh lies in the plane of incidence at asin(t2) from v towards ... T2 = Vh x T1
        th = 0.9
        d = (math.sin(th), 0.0, -math.cos(th))
        r = X.exact_rough_event(d, (0.0, 0.0, 1.0), 1.0, n1, n2, 0.0, 0.6, 0.5)
        vh = (-d[0], 0.0, -d[2])
        t2 = (1.0 - vh[2]) / 2.0
        T2 = (-vh[2] * (vh[0] / abs(vh[0])), 0.0, abs(vh[0]))          # Vh x T1, T1 = (0, Vh.x, 0) / |Vh.x|
        want = [t2 * T2[c] + math.sqrt(1.0 - t2 * t2) * vh[c] for c in range(3)]
        assert max(abs(float(r.m[c]) - want[c]) for c in range(3)) < 1e-15 and r.m[1] == 0
        # the s = -1 half: the same event mirrored in z gives the mirrored m (the basis changes hand, the physics does not)
        a = X.exact_rough_event((0.3, -0.4, -math.sqrt(0.75)), (0.0, 0.0, 1.0), 0.3, n1, n2, 0.4, 0.0, 0.5)
        b = X.exact_rough_event((0.3, -0.4, math.sqrt(0.75)), (0.0, 0.0, 1.0), 0.3, n1, n2, 0.4, 0.0, 0.5)
        assert a.s_sign == 1.0 and b.s_sign == -1.0
        assert abs(a.R - b.R) < 1e-50 and abs(a.m[2] + b.m[2]) < 1e-50
        # total internal reflection about m and the fold: from inside beyond the critical angle, alpha tiny
        r = X.exact_rough_event((math.sin(1.0), 0.0, math.cos(1.0)), (0.0, 0.0, 1.0), 1e-6, 1.5, 1.0, 0.5, 0.3, 0.999)
        assert r.tir and r.R == 1 and r.reflect and r.transmitted is None and r.reflected[2] < 0


def nearest_flip(outcome, lo, hi):
    """The adjacent doubles (a, b), lo <= a < b <= hi, between which outcome(x) changes, by bisection."""
    at_lo = outcome(lo)
    assert at_lo != outcome(hi)
    while math.nextafter(lo, hi) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if outcome(mid) == at_lo else (lo, mid)
    return lo, hi


def floats(v):
    return [float(c) for c in v]


def test_an_ambiguous_ray_is_accepted_either_way_and_still_held_to_the_direction_it_took():
    """No ray of any case is ambiguous, so the branches of `judge_rough` that accept either outcome are run here, on
    events built to sit on each decision: u the double nearest R, a reflected direction in the tangent plane (u_a
    bisected to the pair of doubles between which the fold flips), and q = 1 (u_a bisected to where total internal
    reflection about m sets on)."""
    N, alpha = (0.0, 0.0, 1.0), 0.3
    wrong = [0.6, 0.0, 0.8]
    # |u - R| <= e_R: both kinds are accepted, each with its own direction; a wrong direction is not
    d = (math.sin(0.7), 0.0, -math.cos(0.7))
    R = X.exact_rough_event(d, N, alpha, 1.0, 1.5, 0.4, 0.3, 0.5).R
    r = X.exact_rough_event(d, N, alpha, 1.0, 1.5, 0.4, 0.3, float(R))
    assert r.amb_decision and r.ambiguous and not r.tir
    X.judge_rough("u-on-R", [r], [(True, floats(r.reflected))], "hand")
    X.judge_rough("u-on-R", [r], [(False, floats(r.transmitted))], "hand")
    with pytest.raises(AssertionError):
        X.judge_rough("u-on-R", [r], [(False, floats(r.reflected))], "hand")
    clear = X.exact_rough_event(d, N, alpha, 1.0, 1.5, 0.4, 0.3, 0.5)            # (u well above R: TRANSMIT only)
    assert not clear.ambiguous and not clear.reflect
    with pytest.raises(AssertionError):
        X.judge_rough("u-off-R", [clear], [(True, floats(clear.reflected))], "hand")
    # d'.N within its bound of 0: from inside beyond the critical angle (R = 1: REFLECT whatever u), the reflected
    # direction crosses the tangent plane as u_a grows; at the flip either fold is accepted, a third direction is not
    d = (math.sin(1.0), 0.0, math.cos(1.0))

    def event(ua):
        return X.exact_rough_event(d, N, alpha, 1.5, 1.0, ua, 0.25, 0.5)

    a, b = nearest_flip(lambda ua: event(ua).folded_reflect, 0.0, 0.99)
    seen = set()
    for ua in (a, b):
        r = event(ua)
        assert r.tir and r.reflect and r.amb_fold_reflect and r.ambiguous and not r.amb_decision
        seen.add(r.folded_reflect)
        X.judge_rough("fold", [r], [(True, floats(r.reflected))], "hand")
        X.judge_rough("fold", [r], [(True, floats(r.reflected_other))], "hand")
        with pytest.raises(AssertionError):
            X.judge_rough("fold", [r], [(True, wrong)], "hand")
    assert seen == {True, False}
    r = event(0.5 * a)                                                           # (away from the flip: one fold only)
    assert not r.amb_fold_reflect
    with pytest.raises(AssertionError):
        X.judge_rough("fold", [r], [(True, floats(r.reflected_other))], "hand")
    # |q - 1| <= e_q: from inside near the critical angle of the smooth face; REFLECT and TRANSMIT are both accepted
    # (the transmitted direction exists on either side of the onset: k = sqrt(max(0, .)) = 0 beyond it)
    d = (math.sin(0.73), 0.0, math.cos(0.73))

    def event(ua):
        return X.exact_rough_event(d, N, 0.05, 1.5, 1.0, ua, 0.25, 0.999999)

    a, b = nearest_flip(lambda ua: event(ua).tir, 0.0, 0.99)
    for ua in (a, b):
        r = event(ua)
        assert r.amb_decision and r.ambiguous and r.transmitted is not None
        X.judge_rough("onset", [r], [(True, floats(r.reflected))], "hand")
        X.judge_rough("onset", [r], [(False, floats(r.transmitted))], "hand")
        with pytest.raises(AssertionError):
            X.judge_rough("onset", [r], [(False, wrong)], "hand")


def test_the_judge_of_the_draw_order_needs_each_ray_at_one_position_and_both_positions_taken():
    """`judge_draw_order` on made-up outcomes of twelve events: the replay at positions 2, 3, 4 for some rays and at
    3, 4, 5 for the others passes; all at one position (code that always draws u, or never), a ray that fits neither,
    and a ray with the right direction but the other kind each fail."""
    rng = np.random.default_rng(5)
    v = rng.normal(size=(12, 3))
    v[:, 2] = -np.abs(v[:, 2]) - 0.2
    v /= np.linalg.norm(v, axis=1)[:, None]
    stream = np.array([O.uniforms(SEED + i, 6) for i in range(12)])
    replay = [[X.exact_rough_event(v[i], (0.0, 0.0, 1.0), 0.3, 1.0, 1.5, *stream[i, k:k + 3]) for i in range(12)] for k in (2, 3)]

    def outcome(r):
        return r.reflect, floats(r.reflected if r.reflect else r.transmitted)

    mixed = [outcome(replay[i % 2][i]) for i in range(12)]
    assert X.judge_draw_order("made-up", replay[0], replay[1], mixed, "hand") == (6, 6)
    for k in (0, 1):
        with pytest.raises(AssertionError):
            X.judge_draw_order("made-up", replay[0], replay[1], [outcome(r) for r in replay[k]], "hand")
    with pytest.raises(AssertionError):
        X.judge_draw_order("made-up", replay[0], replay[1], mixed[:5] + [(mixed[5][0], [0.6, 0.0, -0.8])] + mixed[6:], "hand")
    with pytest.raises(AssertionError):
        X.judge_draw_order("made-up", replay[0], replay[1], [(not mixed[0][0], mixed[0][1])] + mixed[1:], "hand")


@pytest.mark.parametrize("case", X.ROUGH_CASES, ids=[c.name for c in X.ROUGH_CASES])
def test_the_host_sampler_agrees_with_the_exact_reference_event_by_event(case):
    _, block, compiled, node_id, pos, dirs, wl, inside, n1, n2, draws = case_inputs(case)
    normals = host_normals(case, block, compiled, node_id, pos, dirs)
    # (the rays meet what the case says they meet: started inside they leave the node, outside they enter it)
    assert np.array_equal(np.sum(normals * dirs, axis=1) > 0.0, inside)
    refs = X.rough_refs(case, dirs, normals, n1, n2, draws, X.TRIG_HOST)
    X.check_rough_conditions(case, refs)
    got = host_events(case, dirs, normals, n1, n2, draws)
    X.judge_rough(case, refs, [(g[0], g[1]) for g in got], "host")
    with mp.workdps(X.DIGITS):
        for i, (r, g) in enumerate(zip(refs, got)):   # (R itself, where it is not 1 by total internal reflection)
            if not r.tir and not r.amb_decision:
                assert abs(mpf(g[3]) - r.R) <= r.e_R, (case, i, g[3], float(r.R), float(r.e_R))
