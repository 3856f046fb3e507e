"""Aligned components without a GPU, exactly and per ray (tests/exact_aligned.py): the lowered directors bit for bit
against item 1 of the PvtAlignTables contract; every `Alignment.emission_table` row against item 1 of the
PvtPhaseTables contract in exact rationals, and what the flattener pools bit for bit against it; the host rule
(`Material.is_absorbed_along`, `.component_along`, `Luminophore.emit`) against the exact restatement within its derived
bound, on the rays tests/test_gpu_aligned_exact.py traces; the kernel-order restatement against the exact one; and the
draw positions and the history judge of the GPU tests on the referee's histories of the twins without alignment.  The
conditions of every case are asserted here from the reference alone, before any GPU run.

Measured on these cases (worst |depth - exact| / bound): the host rule 0.28 (D-plateau; 0.17 to 0.28 over the D, M and
C cases, 0.20 in E-near-zero, 0.03 in E-first-zero), `kernel_step` 0.33 (E-near-zero: a factor near its zero; 0.23 to
0.29 elsewhere); the host's worst |direction - exact| / bound is 0.13 (D-two).  No ray of any case is ambiguous.  The
emission tables' CDF entries are within 61 U of the exact quotient (S_e = 0.6; 0.9 U for S_e = 1 and -0.5), the bound
being (n + j + 6) U >= 520 U.  1.5 * mu * mu in place of 1.5 * (mu * mu) changes the depth of 153 of D-one-S1's 1000 rays."""
from fractions import Fraction as F

import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd import Absorber, Alignment, Box, Material, Node, Ray, Scene
from pvtrace_amd.engine import compile_scene
from pvtrace_amd.material import ALIGN_TABLE_NODES
from tests import exact_aligned as X
from tests import exact_events as XE

IDS = [c.name for c in X.CASES]


def fed(draws):
    """A stand-in for `np.random.uniform` that hands out `draws` in order (a list; it is emptied)."""
    def uniform(low=0.0, high=1.0, size=None):
        if size is None:
            return low + (high - low) * draws.pop(0)
        return np.array([low + (high - low) * draws.pop(0) for _ in range(int(size))])
    return uniform


class Feeding:
    def __init__(self, draws):
        self.draws = draws

    def __enter__(self):
        self.saved = np.random.uniform
        np.random.uniform = fed(self.draws)

    def __exit__(self, *exc):
        np.random.uniform = self.saved


# ---- the restatements on steps worked by hand ----------------------------------------------------------------------------
def test_the_restatements_on_steps_worked_by_hand():
    z = (np.array([0.0, 0.0, 1.0]), 1.0)
    tau = 0.75
    # along a pure dipole: mu = 1, f = 0, the sum is exactly 0 and the depth +inf
    k = X.kernel_step((0, 0, 0), (0.0, 0.0, 1.0), 0.0, [5.0], [z], tau, 0.5)
    assert k.total == 0.0 and k.depth == np.inf and k.factors == [0.0]
    # across it: mu = 0, f = 1.5, depth tau / 7.5, the advance along x
    k = X.kernel_step((0.25, 0, 0), (1.0, 0.0, 0.0), 2.0, [5.0], [z], tau, 0.5)
    assert k.factors == [1.5] and k.depth == 0.1 and np.array_equal(k.position, [0.35, 0.0, 0.0]) and k.travelled == 2.1
    # two components, the second without alignment and not multiplied: sum = 5 * 0.25 + 2 (mu = 1, S = 0.75), p0 = 1.25
    q = (np.array([0.0, 0.0, 1.0]), 0.75)
    k = X.kernel_step((0, 0, 0), (0.0, 0.0, 1.0), 0.0, [5.0, 2.0], [q, None], tau, 1.25 / 3.25)
    assert k.total == 3.25 and k.p0 == 1.25 and k.factors == [0.25, 1.0]
    assert k.component == (0 if np.float64(1.25 / 3.25) * np.float64(3.25) <= 1.25 else 1)
    assert X.kernel_step((0, 0, 0), (0.0, 0.0, 1.0), 0.0, [5.0, 2.0], [q, None], tau, 0.5).component == 1
    # the walk beyond two: partial sums 1.25, 3.25, 4.25
    for u, want in ((0.2, 0), (0.5, 1), (0.9, 2)):
        assert X.kernel_step((0, 0, 0), (0.0, 0.0, 1.0), 0.0, [5.0, 2.0, 1.0], [q, None, None], tau, u).component == want
    # the clamp: a self-dot above 1 is mu = 1, f = 0 exactly -- and without it f would be negative
    n = X.lower_director(np.eye(3), Alignment(X.clamp_director("above")).director)
    assert X.self_dot(n) > 1.0
    assert X.kernel_step((0, 0, 0), n, 0.0, [5.0], [(n, 1.0)], tau, 0.5).total == 0.0
    assert 1.0 - (1.5 * (X.self_dot(n) * X.self_dot(n)) - 0.5) < 0.0
    # the exact restatement of the same steps
    t0, e_t0 = X.exact_exit((0.25, 0, 0), (1.0, 0.0, 0.0), np.eye(4), X.HALF)
    assert t0 == F(3, 4) and e_t0 == 21 * X.U      # 4 ((3 U 0.25 + 0.75 3 U) / 1 + 3 U 0.75)
    r = X.exact_step((1.0, 0.0, 0.0), [5.0], [z], 0.5, 0.5, t0, e_t0)
    assert r.f == [F(3, 2)] and r.total == F(15, 2) and r.absorbed and not r.ambiguous       # ln 2 / 7.5 < 0.75
    assert abs(float(r.depth) - np.log(2.0) / 7.5) < 1e-15 and float(r.bound) < 1e-14
    r = X.exact_step((0.0, 0.0, 1.0), [5.0], [z], 0.5, 0.5, t0, e_t0)
    assert r.total == 0 and not r.absorbed and not r.ambiguous and r.depth == np.inf
    r = X.exact_step((0.0, 0.0, 1.0), [5.0, 2.0, 1.0], [q, None, None], 0.5, 0.5, t0, e_t0)
    assert r.partial == [F(5, 4), F(13, 4), F(17, 4)] and r.component == 1 and r.candidates == {1}
    r = X.exact_step((0.0, 0.0, 1.0), [5.0, 2.0, 1.0], [q, None, None], 0.5, 1.25 / 4.25, t0, e_t0)
    assert r.amb_pick and r.candidates == {0, 1}


# ---- item 1: the lowered directors ------------------------------------------------------------------------------------------
DIRECTORS = [X.GENERIC, X.GENERIC_2, (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0),
             (0.0, 0.0, -1.0), X.MINUS_ZERO, (0.6, -0.0, 0.8), (1e-160, 1.0, 0.0), (1.0, 2.0, 2.0)]


def placed(kind):
    """A scene whose block holds one aligned absorber per director of DIRECTORS -> (scene, block)."""
    world = Node(name="world", geometry=Box((64.0, 64.0, 64.0), material=Material(refractive_index=1.0)))
    comps = [Absorber(1.0, name=f"a{k}", alignment=Alignment(d, 0.5)) for k, d in enumerate(DIRECTORS)]
    parent = world
    if kind == "nested":
        parent = Node(name="parent", parent=world, geometry=Box((8.0, 8.0, 8.0), material=Material(refractive_index=1.0)))
        parent.rotate(*X.PARENT_ROT)
        parent.translate((0.4, -1.1, 2.3))
    block = Node(name="block", parent=parent, geometry=Box((2.0, 2.0, 2.0), material=Material(refractive_index=1.0, components=comps)))
    if kind in ("rotated", "nested"):
        block.rotate(*X.ROT)
    if kind in ("translated", "nested"):
        block.translate((0.3, -0.7, 0.9))
    return Scene(world), block


@pytest.mark.parametrize("kind", ["unrotated", "rotated", "nested", "translated"])
def test_the_lowered_directors_are_item_1_bit_for_bit(kind):
    scene, block = placed(kind)
    compiled = compile_scene(scene)
    node_id = list(compiled.node_names).index(block.name)
    rot = np.asarray(compiled.local_to_world[node_id])[:3, :3]
    if kind in ("unrotated", "translated"):
        assert np.array_equal(rot, np.eye(3))
    else:
        assert not np.any(rot == 0.0)
    comps = block.geometry.material.components
    assert len(compiled.align_axis) == len(DIRECTORS)
    for k, c in enumerate(comps):
        rec = int(compiled.comp_align[int(compiled.comp_start[node_id]) + k])
        want = X.lower_director(rot, c.alignment.director)
        got = np.asarray(compiled.align_axis[rec])
        assert np.array_equal(got, want), (kind, DIRECTORS[k], got, want)
        assert np.array_equal(np.signbit(got), np.signbit(want)), (kind, DIRECTORS[k], "the sign of a zero")
        assert abs(X.self_dot(got) - 1.0) <= 4 * 2.0 ** -53
    if kind == "unrotated":
        k = DIRECTORS.index(X.MINUS_ZERO)
        z = compiled.align_axis[int(compiled.comp_align[int(compiled.comp_start[node_id]) + k])][2]
        assert z == 0.0 and np.signbit(z)                               # n_w.z = -0.0: s = -1 in Duff's basis
        k = DIRECTORS.index((1e-160, 1.0, 0.0))
        assert list(compiled.align_axis[int(compiled.comp_align[int(compiled.comp_start[node_id]) + k])]) == [1e-160, 1.0, 0.0]


# ---- the emission tables ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1.0, -0.5, 0.6, 1e-3, -1e-3])
def test_every_emission_table_row_is_item_1_of_the_phase_tables_contract(order):
    table = Alignment((0.0, 0.0, 1.0), 0.0, order).emission_table
    n = ALIGN_TABLE_NODES
    assert table.cdf.shape == (1, n) and table.mu.shape == (n,) and table.wavelength is None
    assert table.mu[0] == -1.0 and table.mu[-1] == 1.0 and table.cdf[0, 0] == 0.0 and table.cdf[0, -1] == 1.0
    assert np.all(np.diff(table.cdf[0]) >= 0.0)
    h = F(2, n - 1)
    for k in range(n):   # uniform within 1 ulp of the node's exact place
        assert abs(F(float(table.mu[k])) - (-1 + k * h)) <= F(float(np.spacing(max(abs(table.mu[k]), 2.0 ** -9)))), k
    # the tabulated values are f(mu; S_e) by the rule's own operations, never negative
    assert np.array_equal(table.values[::-1], np.maximum(1.0 - order * (1.5 * (table.mu * table.mu) - 0.5), 0.0))
    worst = XE.check_cdf_rows(table, order)
    print(f"S_e = {order}: worst |C_j - exact| / (U exact) {worst:.2f}")


def test_the_pooled_phase_table_of_a_record_is_its_alignments_table_bit_for_bit():
    for name in ("D-one-S1", "D-two", "D-rotated", "D-mesh"):
        x = X.inputs(X.BY_NAME[name])
        c = x.compiled
        for k, emitter in enumerate(x.emitters):
            rec = int(c.comp_align[x.cbase + k])
            if emitter is None:
                assert rec < 0 or c.align_emit_table[rec] == -1
                continue
            t = int(c.align_emit_table[rec])
            assert t >= 0 and t == int(c.comp_phase_table[x.cbase + k]) and c.ptab_nw[t] == 1 and c.ptab_nmu[t] == ALIGN_TABLE_NODES
            table = emitter[1]
            m, s = int(c.ptab_mu_start[t]), int(c.ptab_cdf_start[t])
            assert np.array_equal(c.ptab_mu[m:m + ALIGN_TABLE_NODES], table.mu)
            assert np.array_equal(c.ptab_cdf[s:s + ALIGN_TABLE_NODES], table.cdf[0])
            assert c.align_abs_order[rec] == x.case.comps[k]["s_a"]


# ---- the cases: conditions, the kernel-order restatement, the host rule ----------------------------------------------------
@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_the_conditions_hold_and_the_kernel_order_restatement_lies_within_the_exact_bound(case):
    x = X.inputs(case)
    refs = X.first_refs(case)
    X.check_conditions(case, refs)
    worst = 0.0
    for i, r in enumerate(refs):
        k = X.kernel_step(x.pos[i], x.dirs[i], 0.0, x.alphas(x.wl[i]), x.records, x.taus[i, 0], x.draws[i, 1])
        with X.precise:
            if np.isfinite(k.depth) and r.bound != np.inf:
                ratio = float(abs(X.mpf(k.depth) - r.depth) / r.bound)
                assert ratio <= 1.0, (case, i, k.depth, float(r.depth), ratio)
                worst = max(worst, ratio)
            else:
                assert X.mpf(k.depth) >= r.depth_lo, (case, i, k.depth, float(r.depth_lo))
            if not r.amb_depth:
                assert (X.mpf(k.depth) < X.to_mpf(r.t0)) == r.absorbed, (case, i)
        if r.absorbed and not r.ambiguous:
            assert k.component == r.component, (case, i, k.component, r.component)
    print(f"{case}: kernel_step worst |depth - exact| / bound {worst:.3f}")


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_the_host_rule_agrees_with_the_exact_reference_ray_by_ray(case):
    x = X.inputs(case)
    medium = x.block.geometry.material
    directors = [None if c.alignment is None else c.alignment.director for c in medium.components]
    for wl in set(x.wl):
        assert [float(c.coefficient(wl)) for c in medium.components] == x.alphas(wl), (case, wl)
    worst, ambiguous, absorbed_n = 0.0, 0, 0
    for i in range(case.n):
        frame = X.frame_cosines(x.dirs[i], x.w2l, directors)
        t0, e_t0 = X.exact_exit(x.pos[i], x.dirs[i], x.w2l, X.HALF)
        r = X.exact_step(x.dirs[i], x.alphas(x.wl[i]), x.records, x.draws[i, 0], x.draws[i, 1], t0, e_t0, frame=frame)
        local = Ray(tuple(x.pos[i]), tuple(x.dirs[i]), float(x.wl[i])).representation(x.scene.root, x.block)
        draws = [float(x.draws[i, 0])]
        with Feeding(draws):
            absorbed, depth = medium.is_absorbed_along(local, float(t0))
        assert not draws
        ambiguous += r.ambiguous
        with X.precise:
            if not r.amb_depth:
                assert bool(absorbed) == r.absorbed, (case, i, "absorbed", absorbed, float(r.depth), float(t0))
            if np.isfinite(depth) and r.bound != np.inf:
                ratio = float(abs(X.mpf(float(depth)) - r.depth) / r.bound)
                assert ratio <= 1.0, (case, i, "depth", depth, float(r.depth), ratio)
                worst = max(worst, ratio)
            else:
                assert X.mpf(float(depth)) >= r.depth_lo, (case, i, depth, float(r.depth_lo))
        if absorbed:
            absorbed_n += 1
            draws = [float(x.draws[i, 1])]
            with Feeding(draws):
                k = medium.components.index(medium.component_along(float(x.wl[i]), local.direction))
            assert not draws
            assert (k in r.candidates) if r.amb_pick else k == r.component, (case, i, "pick", k, r.component)
    print(f"{case}: host worst |depth - exact| / bound {worst:.3f}; absorbed {absorbed_n}; ambiguous {ambiguous} of {case.n}")
    assert ambiguous * 100 <= case.n, (case, ambiguous)


EMITTING = ["D-one-S1", "D-one-planar", "D-two", "D-rotated", "D-mesh", "M-cone5"]


@pytest.mark.parametrize("name", EMITTING)
def test_the_host_emission_turns_about_the_director_and_keeps_the_wavelength_draw(name):
    """`Luminophore.emit` on the aligned dye, fed draws 3, 4 and 5 of every ray's stream (u2, u3 and the wavelength's):
    the direction against `exact_phase_turn` about the director of the node's frame, which is the frame the host emits
    in, under TRIG_HOST; the wavelength equal to the S_e = 0 twin's under the same draws."""
    case = X.BY_NAME[name]
    x = X.inputs(case)
    k = next(k for k, e in enumerate(x.emitters) if e is not None)
    dye = x.block.geometry.material.components[k]
    twin = case.components(emission=False)[k]
    assert dye.alignment.emission_order != 0.0 and twin.alignment.emission_order == 0.0
    refs, got = [], []
    for i in range(case.n):
        local = Ray(tuple(x.pos[i]), tuple(x.dirs[i]), float(x.wl[i])).representation(x.scene.root, x.block)
        u = [float(v) for v in x.draws[i, 3:6]]
        draws = list(u)
        with Feeding(draws):
            out = dye.emit(local)
        assert not draws
        draws = list(u)
        with Feeding(draws):
            plain = twin.emit(local)
        assert not draws
        assert out.wavelength == plain.wavelength and out.wavelength != local.wavelength, (name, i)
        refs.append(XE.exact_phase_turn(dye.alignment.emission_table, local.wavelength, dye.alignment.director, 0.0, u[0], u[1],
                                        trig=XE.TRIG_HOST))
        got.append(np.asarray(out.direction, dtype=np.float64))
    assert not any(r.ambiguous for r in refs)
    XE.judge_phase(case, refs, got, "host")


# ---- the bit-for-bit assertion sees an operation order ------------------------------------------------------------------------
def test_a_changed_operation_order_changes_the_kernel_order_restatement():
    """The host rule is judged within a bound, which no operation order can fail; the kernel is judged with `==`
    against `kernel_step`.  That `==` sees 1.5 * mu * mu in place of 1.5 * (mu * mu): the two differ in the depth of
    more than a tenth of a D case's rays."""
    case = X.BY_NAME["D-one-S1"]
    x = X.inputs(case)
    differ = 0
    for i in range(case.n):
        args = (x.pos[i], x.dirs[i], 0.0, x.alphas(x.wl[i]), x.records, x.taus[i, 0], x.draws[i, 1])
        differ += X.kernel_step(*args).depth != X.kernel_step(*args, order="left").depth
    print(f"1.5 * mu * mu changes the depth of {differ} of {case.n} rays")
    assert differ * 10 >= case.n


# ---- the draw positions and the judge, on the referee's histories of the twins without alignment ----------------------------
def referee_history(x):
    data = O.trace_bundle(x.compiled, x.pos, x.dirs, x.wl, X.SEED, X.MAXSTEPS, X.ME, 0, 4, 1, math_mode=O.MATH_PORTABLE)
    return X.History(data, x.case.n)


@pytest.mark.parametrize("name", ["D-one-S1", "D-two", "D-three", "C-two", "C-bounce", "D-rotated"])
def test_the_twin_without_alignment_is_judged_bit_for_bit_on_the_referees_histories(name):
    """The referee traces the unaligned twins bit for bit as the kernel does, so the draw positions (0 and 6 k along a
    luminophore's chain, 2 m after m reflections, the pick one behind) and `judge_history` itself are proven here:
    with no record, `kernel_step` is the plain law."""
    case = X.BY_NAME[name]
    x = X.inputs(case, aligned=False)
    assert all(r is None for r in x.records) and not x.compiled.has_alignment
    j = X.judge_history(x, referee_history(x), "referee")
    print(f"{case} twin: {j.absorptions} first-step and {j.later} later-step ABSORB rows held, {j.not_absorbed} steps to the surface")
    assert j.absorptions * 10 >= 2 * case.n
    if case.family == "C" or name == "D-one-S1":
        assert j.later >= 300 and j.later_turned >= 100, (name, j.later, j.later_turned)
