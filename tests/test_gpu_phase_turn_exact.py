"""The kernel's phase-table turn (`phase_table_turn`, `phase_table_turn_call`, pvt_trace_kernel.h) against the exact
reference of the PvtPhaseTables contract (tests/exact_events.py), one turn at a time.

A host ray started inside a block of one table component draws, in the order of its stream `seed + index`: 0 the free
path, 1 the component pick, 2 the quantum yield, then u1 (only when the table has several rows), u2 and u3.  The SCATTER
(or EMIT) row that follows the ABSORB row holds the new direction; the incoming one is the direction as launched.  The
anchor tests fix those positions on the same blocks with an ISOTROPIC phase function, bit for bit: the depth of the
ABSORB row from draw 0 and the referee's isotropic direction from draws 3 and 4.  The table cases (tests/exact_events.py;
its case table says which reaches the inlined turn, the called turn, the called turn of a mesh scene, the LDS copy and
the global-memory copy of a table) then hold the direction to the reference within the derived bound, and a table
luminophore's EMIT wavelength to the same scene with an isotropic phase function: the draw order of item 5.  Rays that
leave without being absorbed are not judged.  The same rays hold the host sampler in tests/test_phase_turn_exact.py.

Measured on an MI355X (worst |direction - exact| / bound): 0.113 (the 1801-point g = 0.9 table); no ray of any
case is ambiguous (docs/parity_chain.md, tabulated phase functions)."""
import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd.engine import Session, compile_scene
from pvtrace_amd.engine.compiler import PHASE_ISOTROPIC
from tests import exact_events as X
from tests.test_phase_turn_exact import FIRST_PHASE_DRAW, SEED, case_inputs

pytestmark = pytest.mark.gpu

GENERATE, ABSORB, SCATTER, EMIT = 0, 3, 5, 6
ME = 4
ALPHA = 5.0   # the component's coefficient (PhaseCase.scene)


LDS_BUDGET = 64 * 1024   # plan_lds (pvt_trace.hip): what a workgroup's accumulators, queues and staged tables may take


def turn_events(scene, pos, dirs, wl, launch=None):
    """Of every ray: whether its first event is an ABSORB that a row follows, that row's kind, direction and
    wavelength, and the ABSORB row's `travelled`.  `launch`: a dict that receives the launch's `launch_info()`."""
    n = len(pos)
    with Session(scene, emission="host") as session:
        result = session.collect(session.submit(n, SEED, host_rays=(pos, dirs, wl, ["r"] * n), record_every=1,
                                                max_events=ME))
        data = {k: np.asarray(result.data[k]).copy() for k in ("counts", "kind", "direction", "wavelength", "travelled")}
        if launch is not None:
            launch.update(session.dscene.launch_info())
    first = np.arange(n) * ME
    assert np.all(data["counts"] >= 2) and np.all(data["kind"][first] == GENERATE)
    absorbed = (data["kind"][first + 1] == ABSORB) & (data["counts"] >= 3)
    return (absorbed, data["kind"][first + 2], data["direction"].reshape(-1, 3)[first + 2], data["wavelength"][first + 2],
            data["travelled"][first + 1])


def isotropic(g1, g2):
    """The built-in isotropic direction from its two draws, in the kernel's operations (the referee's portable math)."""
    c = 2.0 * g2 - 1.0
    s = O.math("sqrt1m2", c)
    return np.column_stack([s * O.math("cos2pi", g1), s * O.math("sin2pi", g1), c])


def test_the_isotropic_formula_is_the_referees():
    for seed in (1, 77, 4242):
        g = O.uniforms(seed, 2)
        assert np.array_equal(isotropic(g[:1], g[1:2])[0], O.phase(PHASE_ISOTROPIC, 0.0, seed, O.MATH_PORTABLE))


ANCHORS = ["P-constant", "P-two-row-wide-inlined", "P-two-row-mesh", "P-rayleigh-luminophore"]


@pytest.mark.parametrize("name", ANCHORS)
def test_anchor_an_isotropic_component_turns_with_draws_three_and_four(name):
    case = X.PHASE_BY_NAME[name]
    pos, dirs, wl = case.rays()
    scene, _ = case.scene(tabled=False)
    absorbed, kind, direction, _, travelled = turn_events(scene, pos, dirs, wl)
    draws = np.array([O.uniforms(SEED + i, FIRST_PHASE_DRAW + 2) for i in range(case.n)])
    assert absorbed.sum() * 10 >= 4 * case.n
    assert np.all(kind[absorbed] == (EMIT if case.component == "luminophore" else SCATTER))
    depth = -O.math("log", 1.0 - draws[:, 0]) / ALPHA                       # draw 0 (div_normal is the IEEE quotient)
    assert np.array_equal(travelled[absorbed], depth[absorbed])              # bit for bit
    want = isotropic(draws[:, FIRST_PHASE_DRAW], draws[:, FIRST_PHASE_DRAW + 1])
    assert np.array_equal(direction[absorbed], want[absorbed])               # bit for bit


@pytest.mark.parametrize("case", X.PHASE_CASES, ids=[c.name for c in X.PHASE_CASES])
def test_the_kernel_turn_agrees_with_the_exact_reference_ray_by_ray(case):
    pos, dirs, wl, u1, u2, u3 = case_inputs(case)
    scene, _ = case.scene()
    compiled = compile_scene(scene)
    # the path the case table names.  More than 64 recorders (SEENW = 4) without a mesh inline the turn, a mesh scene is
    # the "mesh" family; the table -- its wavelengths, mu axis and CDF rows -- is staged in LDS with all the scene's
    # tables or not at all (these scenes have no other spectrum), so it is staged only where it is within plan_lds's
    # budget AND within what the launch actually reserved, and read from global memory where it exceeds either.
    table_bytes = 8 * (case.table.cdf.size + case.table.mu.size + case.table.n_wavelength + 2)
    launch = {}
    absorbed, kind, direction, wavelength, _ = turn_events(scene, pos, dirs, wl, launch=launch)
    assert (len(compiled.rec_node) > 64) == (case.container == "wide")
    assert (launch["variant"] == "mesh") == (case.container == "mesh")
    fits = table_bytes <= LDS_BUDGET and table_bytes <= launch["lds_bytes"]
    assert fits == (case.table_key != "hg-1801x20"), (case, table_bytes, launch)
    assert table_bytes > LDS_BUDGET or case.table_key != "hg-1801x20"       # (the global-memory case exceeds the budget itself)
    assert np.all(kind[absorbed] == (EMIT if case.component == "luminophore" else SCATTER))
    refs = X.phase_refs(case, dirs, wl, u1, u2, u3, X.TRIG_KERNEL)
    X.check_phase_conditions(case, refs, judged=absorbed)
    X.judge_phase(case, refs, [direction[i] if absorbed[i] else None for i in range(case.n)], "kernel")
    if case.component == "luminophore":
        plain, _ = case.scene(tabled=False)
        absorbed0, kind0, _, wavelength0, _ = turn_events(plain, pos, dirs, wl)
        assert np.array_equal(absorbed, absorbed0) and np.all(kind0[absorbed0] == EMIT)
        assert np.array_equal(wavelength[absorbed], wavelength0[absorbed])   # the wavelength draw follows u2 and u3
        assert np.any(wavelength[absorbed] != wl[absorbed])
    else:
        assert np.array_equal(wavelength[absorbed], wl[absorbed])
