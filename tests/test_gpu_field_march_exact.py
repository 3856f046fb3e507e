"""The kernel's concentration-field march (`field_march_call`, pvt_trace_kernel.h) against the exact rational reference
of the contract (tests/exact_march.py), ray by ray.

A host ray started inside a fielded node draws u0 for tau* = -pvt_log(1 - u0) and, if absorbed, u1 for the component:
the first two uniforms of its stream `seed + index`.  The ABSORB row's `travelled` is 0 + the march's depth, bit for
bit, and `component` is the pick, so one step and two draws are replayed, nothing else.  The anchor tests fix the draw
positions on the same blocks WITHOUT a field, bit for bit; the fielded cases (tests/exact_march.py: generic rays and
exact ties, four component layouts, the analytic box, a tile of a node-grid scene and a 12-triangle mesh) then hold
absorbed-or-not, depth, component and position to the reference within the derived bound.  The same rays hold the host
march in tests/test_field_march_exact.py.

Measured on an MI355X (worst |depth - exact| / bound): 0.18 in family A, 0.18 in family B, no ray ambiguous; position
error / its bound at most 0.94 (docs/parity_chain.md, concentration fields)."""
from fractions import Fraction as F

import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd.engine import Session
from tests import exact_march as X
from tests.test_field_march_exact import SEED, case_inputs, judge

pytestmark = pytest.mark.gpu

GENERATE, TRANSMIT, ABSORB, EXIT = 0, 2, 3, 7
ME = 4


def first_events(scene, pos, dirs, wavelength):
    """The first event after GENERATE of every ray: (kind, travelled, component, position)."""
    n = len(pos)
    wl = np.full(n, float(wavelength))
    with Session(scene, emission="host") as session:
        result = session.collect(session.submit(n, SEED, host_rays=(pos, dirs, wl, ["r"] * n), record_every=1,
                                                max_events=ME))
        data = {k: np.asarray(result.data[k]).copy() for k in ("counts", "kind", "travelled", "component", "position")}
    assert np.all(data["counts"] >= 2)
    first = np.arange(n) * ME
    assert np.all(data["kind"][first] == GENERATE)
    return (data["kind"][first + 1], data["travelled"][first + 1], data["component"][first + 1],
            data["position"].reshape(-1, 3)[first + 1])


def kernel_tau(u0):
    """tau* = -pvt_log(1 - u0), the kernel's bits (the referee's portable logarithm)."""
    return -O.math("log", 1.0 - u0)


ANCHORS = ["A-357-three-box-rotated", "A-119-two-tile", "A-612-field-and-plain-mesh-rotated"]


@pytest.mark.parametrize("name", ANCHORS)
def test_anchor_an_unfielded_block_draws_u0_for_the_depth_and_u1_for_the_component(name):
    case = X.CASE_BY_NAME[name]
    _, _, compiled, node_id, pos, dirs, u0, u1 = case_inputs(case)      # (the fielded scene: the same rays)
    scene, _ = case.scene(fielded=False)
    kind, travelled, component, _ = first_events(scene, pos, dirs, case.wavelength)
    alphas = case.alphas()
    alpha, partial = 0.0, []
    for a in alphas:
        alpha += a
        partial.append(alpha)
    depth = kernel_tau(u0) / alpha                                        # (div_normal is the IEEE quotient)
    t0 = np.array([float(X.exact_march(pos[i], dirs[i], compiled.world_to_local[node_id], case.lower, case.upper,
                                       (1, 1, 1), [None] * len(alphas), alphas, 1.0, 0.5, case.half).t0)
                   for i in range(case.n)])
    absorbed = kind == ABSORB
    clear = np.abs(depth - t0) > 1e-9
    assert np.array_equal(absorbed[clear], (depth < t0)[clear])
    assert 0.2 * case.n < absorbed.sum() < 0.95 * case.n
    assert np.all(np.isin(kind[~absorbed], (TRANSMIT, EXIT)))
    assert np.array_equal(travelled[absorbed], depth[absorbed])           # bit for bit
    target = u1 * alpha
    want = np.zeros(case.n, dtype=int)
    for i in range(case.n):
        for k, running in enumerate(partial):
            if target[i] <= running:
                want[i] = k
                break
    got = component - int(compiled.comp_start[node_id])
    assert np.array_equal(got[absorbed], want[absorbed])
    assert len(set(want[absorbed].tolist())) == len(alphas)


@pytest.mark.parametrize("case", X.CASES, ids=[c.name for c in X.CASES])
def test_the_kernel_march_agrees_with_the_exact_reference_ray_by_ray(case):
    scene, _, compiled, node_id, pos, dirs, u0, u1 = case_inputs(case)
    taus = kernel_tau(u0)
    refs = X.references(case, compiled, node_id, pos, dirs, taus, u1)
    kind, travelled, component, where = first_events(scene, pos, dirs, case.wavelength)
    absorbed = kind == ABSORB
    assert np.all(np.isin(kind[~absorbed], (TRANSMIT, EXIT)))
    first = int(compiled.comp_start[node_id])
    got = [(bool(absorbed[i]), float(travelled[i]), None, int(component[i]) - first) for i in range(case.n)]
    judge(case, refs, got, "kernel")
    worst = 0.0
    for i, r in enumerate(refs):
        if not (absorbed[i] and r.absorbed):
            continue
        for c in range(3):
            x, v = F(float(pos[i, c])), F(float(dirs[i, c]))
            want = x + v * r.depth
            tol = abs(v) * r.bound + X.U * abs(v * r.depth) + X.U * abs(want)
            err = abs(F(float(where[i, c])) - want)
            assert err <= tol, (case, i, c, float(where[i, c]), float(want), float(err), float(tol))
            if tol:
                worst = max(worst, float(err / tol))
    print(f"kernel {case}: worst |position - exact| / bound {worst:.3f}")
