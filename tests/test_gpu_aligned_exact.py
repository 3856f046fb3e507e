"""The kernel's aligned step (`align_factor`, `align_scale_call`, `align_term`, `align_axis`, pvt_trace_kernel.h)
against the exact references of the PvtAlignTables contract (tests/exact_aligned.py), ray by ray.

Every ray is a host ray that starts INSIDE the aligned block; ray i draws from the stream SEED + i; every launch logs
every event (record_every = 1, max_events = 16, maxsteps = 64).  The anchors come first: on the twins WITHOUT alignment
they fix, bit for bit, the draw positions the aligned cases rely on -- the first and the second ABSORB of a
one-luminophore block from draws 0 and 6, the ABSORB after a REFLECT inside an index-1.5 block from draw 2, the pick of
a two-component block from draw 1 (tests/test_aligned_exact.py proves the same on the referee's histories without a
GPU).  Then every case: each ABSORB row is held with `==` to `kernel_step` on the PRECEDING row's direction, position,
`travelled` and wavelength as logged (family D: the first step; E: the edges; C: the later steps of item 9, after a
re-emission or a reflection, and rays of both kinds launched alone through the tail function), absorbed-or-not and the pick
to `exact_step`, and every first EMIT row (the second too along C-lum's chains) to `exact_phase_turn` about n_w within
its bound, its wavelength to the S_e = 0 twin's.  The conditions of a case are asserted from the reference alone.

Measured on an MI355X: every ABSORB row of every case equal to `kernel_step` value for value (first steps: all the
reference absorbs, 752 to 1126 per D, M and C case, 822 in E-first-zero, 143 in E-near-zero, none in E-clamp; later steps:
1919 in C-lum, 1557 in C-two, 733 in C-bounce); no step of any case ambiguous; worst |direction - exact| / bound 0.113
(C-lum, first and second emissions; 0.087 to 0.104 in the other cases) (docs/parity_chain.md, aligned luminophores)."""
import numpy as np
import pytest

from pvtrace_amd.engine import Session, native
from tests import exact_aligned as X

pytestmark = pytest.mark.gpu

COLUMNS = ("counts", "kind", "container", "component", "position", "direction", "wavelength", "travelled")
IDS = [c.name for c in X.CASES]


def trace(scene, pos, dirs, wl, launch=None, ray_offset=0):
    """The histories of one launch -> `History`.  `launch`: a dict that receives the launch's `launch_info()`."""
    n = len(pos)
    with Session(scene, emission="host") as session:
        result = session.collect(session.submit(n, X.SEED, host_rays=(pos, dirs, wl, ["r"] * n), record_every=1,
                                                max_events=X.ME, maxsteps=X.MAXSTEPS, ray_offset=ray_offset))
        data = {k: np.asarray(result.data[k]).copy() for k in COLUMNS}
        if launch is not None:
            launch.update(session.dscene.launch_info())
    return X.History(data, n)


def live(hist):
    return np.arange(hist.me)[None, :] < hist.counts[:, None]


# ---- the anchors: the twins without alignment ------------------------------------------------------------------------------
def test_anchor_the_first_and_the_second_absorb_of_a_luminophore_block_draw_at_0_and_6():
    case = X.BY_NAME["C-lum"]
    x = X.inputs(case, aligned=False)
    hist = trace(x.scene, x.pos, x.dirs, x.wl)
    first = hist.kind[:, 1] == X.ABSORB
    assert first.sum() * 10 >= 4 * case.n
    assert np.array_equal(hist.travelled[first, 1], (x.taus[:, 0] / 5.0)[first])                     # draw 0
    second = first & (hist.counts >= 4) & (hist.kind[:, 2] == X.EMIT) & (hist.kind[:, 3] == X.ABSORB)
    assert second.sum() >= 300
    assert np.array_equal(hist.travelled[second, 3], (hist.travelled[:, 2] + x.taus[:, 6] / 5.0)[second])   # draw 6
    j = X.judge_history(x, hist, "kernel, no alignment", max_absorptions=3)
    assert j.absorptions == first.sum() and j.later >= 300


def test_anchor_the_absorb_after_a_reflect_inside_the_glass_block_draws_at_2():
    case = X.BY_NAME["C-bounce"]
    x = X.inputs(case, aligned=False)
    hist = trace(x.scene, x.pos, x.dirs, x.wl)
    after = (hist.counts >= 3) & (hist.kind[:, 1] == X.REFLECT) & (hist.kind[:, 2] == X.ABSORB)
    assert after.sum() >= 100
    assert np.all(hist.container[after, 1] == x.node_id)
    alpha = x.alphas(555.0)[0]
    assert np.array_equal(hist.travelled[after, 2], (hist.travelled[:, 1] + x.taus[:, 2] / alpha)[after])   # draw 2
    j = X.judge_history(x, hist, "kernel, no alignment", max_steps=6)
    assert j.later >= 300


def test_anchor_the_pick_of_a_two_component_block_draws_at_1():
    case = X.BY_NAME["D-two"]
    x = X.inputs(case, aligned=False)
    hist = trace(x.scene, x.pos, x.dirs, x.wl)
    first = hist.kind[:, 1] == X.ABSORB
    a0, a1 = x.alphas(555.0)
    total = a0 + a1
    assert np.array_equal(hist.travelled[first, 1], (x.taus[:, 0] / total)[first])
    want = np.where(x.draws[:, 1] * total <= a0, 0, 1) + x.cbase
    assert np.array_equal(hist.component[first, 1], want[first]) and len(set(want[first])) == 2     # draw 1
    X.judge_history(x, hist, "kernel, no alignment", max_absorptions=1)


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def first_emit_wavelengths(hist):
    """Per ray the wavelength of the row after a first-step ABSORB when that row is an EMIT, else NaN."""
    emitted = (hist.counts >= 3) & (hist.kind[:, 1] == X.ABSORB) & (hist.kind[:, 2] == X.EMIT)
    return np.where(emitted, hist.wavelength[:, 2], np.nan)


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_the_kernel_step_agrees_with_the_contract_ray_by_ray(case):
    x = X.inputs(case)
    refs = X.first_refs(case)
    n_absorbed, n_ambiguous, _ = X.check_conditions(case, refs)
    launch = {}
    hist = trace(x.scene, x.pos, x.dirs, x.wl, launch=launch)
    # the path: every scene with an aligned component runs the extension family; the wide case has the four-word seen
    # mask (the inlined turn), the tile case is filed in a node grid
    assert x.compiled.has_alignment and launch["variant"] == "rough", launch
    assert (len(x.compiled.rec_node) > 64) == (case.container == "wide")
    assert (native.node_grid_plan(x.compiled) is not None) == (case.container == "tile")
    if case.container == "tile":
        assert len(x.compiled.node_names) == 10
    limits = dict(max_steps=6) if case.name == "C-bounce" else dict(max_absorptions=3 if case.family == "C" else 1)
    j = X.judge_history(x, hist, "kernel", **limits)
    print(f"kernel {case}: {j.absorptions} first-step and {j.later} later-step ABSORB rows equal to kernel_step, "
          f"{j.not_absorbed} steps to the surface, {j.ambiguous} ambiguous steps, {len(j.emissions)} EMIT rows")
    if n_ambiguous == 0:
        assert j.absorptions == n_absorbed, (case, j.absorptions, n_absorbed)
    if case.name.startswith("E-clamp"):
        rows = live(hist)
        assert not np.any((hist.kind == X.ABSORB) & rows)                                # no history holds an ABSORB row ...
        assert np.all(hist.kind[np.arange(case.n), hist.counts - 1] == X.EXIT)           # ... and every one ends in EXIT
        twin = X.inputs(case, aligned=False)                                             # the zero is the alignment's:
        bare = trace(twin.scene, twin.pos, twin.dirs, twin.wl)                           # the twin absorbs 1 - exp(-alpha chord)
        jt = X.judge_history(twin, bare, "kernel, no alignment", max_absorptions=1)
        assert jt.absorptions * 10 >= 4 * case.n, (case, jt.absorptions)
    if case.name == "E-first-zero":
        first = hist.kind[:, 1] == X.ABSORB
        alpha1 = x.alphas(555.0)[1]
        assert np.all(hist.component[first, 1] == x.cbase + 1)
        assert np.array_equal(hist.travelled[first, 1], (x.taus[:, 0] / alpha1)[first])
    if case.family == "C":
        assert j.later >= 300 and j.later_turned >= 100, (case, j.later, j.later_turned)
    emissions = [e for e in j.emissions if e[1] == 0 or case.name == "C-lum"]
    if any(c["s_e"] != 0.0 for c in case.comps):
        assert len(emissions) * 10 >= 3 * case.n, (case, len(emissions))
        worst = X.judge_emissions(case, emissions, "kernel")
        assert worst < 1.0
        if case.name == "C-lum":
            assert sum(e[1] > 0 for e in emissions) >= 300
        # the wavelength draw follows u2 and u3: the EMIT wavelength is the S_e = 0 twin's, ray for ray
        plain, _ = case.scene(emission=False)
        twin = first_emit_wavelengths(trace(plain, x.pos, x.dirs, x.wl))
        mine = first_emit_wavelengths(hist)
        assert np.array_equal(mine, twin, equal_nan=True) and np.sum(~np.isnan(mine)) * 10 >= 3 * case.n
        assert np.any(mine[~np.isnan(mine)] != x.wl[~np.isnan(mine)])
    else:
        assert not j.emissions
    if case.name in ("C-lum", "C-bounce"):
        # C-tail: eight rays with at least two later absorptions (C-lum), or with an absorption after at least two
        # reflections (C-bounce: a reflection keeps the wavelength, so the tail function's cache of UNSCALED sums, keyed by
        # container and wavelength, is what the step finds), each launched alone -- the tail function finishes a launch
        # of one: the same rows, held by the same reference
        need = 2 if case.name == "C-lum" else 3
        chosen = [i for i, rows in sorted(j.chains.items()) if (len(rows) if case.name == "C-lum" else rows[0]) >= need][:8]
        assert len(chosen) == 8
        for i in chosen:
            alone = trace(x.scene, x.pos[i:i + 1], x.dirs[i:i + 1], x.wl[i:i + 1], ray_offset=i)
            count = int(hist.counts[i])
            assert alone.counts[0] == count
            for key in ("kind", "container", "component", "position", "direction", "wavelength", "travelled"):
                assert np.array_equal(getattr(alone, key)[0, :count], getattr(hist, key)[i, :count]), (case, i, key)
            ja = X.judge_history(X.subset(x, [i]), alone, "kernel, alone", **limits)
            assert ja.later >= (2 if case.name == "C-lum" else 1)
