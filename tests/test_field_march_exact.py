"""The host's concentration-field march (`material._march` through `Material.is_absorbed_in / component_at`) against the
exact rational reference of the contract (tests/exact_march.py), ray by ray, on both ray families: generic rays (A)
and exact ties on planes, edges and vertices (B).  The same cases, rays and draws hold the kernel in
tests/test_gpu_field_march_exact.py; here the reference, its margins and the share of ambiguous rays are proven
without a GPU.

Measured on these cases (worst |depth - exact| / bound): 0.23 in family A, 0.18 in family B, no ray ambiguous.  The
error stays within 2.3 ulp of max(depth, t0) in the unrotated cases, but for family B's dense-before-thin cells (8.7 ulp)
and reaches 554 ulp in a rotated node for a ray nearly parallel to a plane it crosses: what the bound's terms are for."""
from fractions import Fraction as F

import numpy as np
import pytest

from oracle import oracle as O
from pvtrace_amd import Ray
from pvtrace_amd.engine import compile_scene
from tests import exact_march as X

SEED = 4100


def case_inputs(case):
    """(scene, block, compiled, node id, world positions, directions, u0, u1) of a case: the two uniforms are the first
    two of each ray's stream, as the kernel draws them."""
    scene, block = case.scene()
    compiled = compile_scene(scene)
    node_id = list(compiled.node_names).index(block.name)
    pos, dirs = case.world_rays(compiled, node_id)
    draws = np.array([O.uniforms(SEED + i, 2) for i in range(case.n)])
    return scene, block, compiled, node_id, pos, dirs, draws[:, 0], draws[:, 1]


def test_the_spectrum_of_the_cases_is_looked_up_exactly_by_host_and_referee():
    from pvtrace_amd import Absorber
    comp = Absorber(X.SPECTRUM)
    for wl in (480.0, 650.0, 384.0, 512.0, 768.0):
        want = X.spectral_alpha(wl)
        assert F(float(comp.coefficient(wl))) == want, wl
        assert F(O.interp(wl, X.SPECTRUM[:, 0], X.SPECTRUM[:, 1])) == want, wl


def test_the_reference_on_rays_worked_by_hand():
    """A 1 x 1 x 4 lattice on [-1, 1]^3 in a 3 cm box, values 1, 0, 2, 0.5, alpha 1: a ray up the z axis from z = -1.25
    has tau(s) = s on [0, 0.75] (edge cell, clamped), 0 on the clear cell, then 2 (s - 1.25) ..."""
    vals = [np.array([1.0, 0.0, 2.0, 0.5]).reshape(1, 1, 4)]
    eye = np.eye(4)
    args = dict(w2l=eye, lower=(-1, -1, -1), upper=(1, 1, 1), shape=(1, 1, 4), values=vals, alphas=[1.0], u1=0.5,
                half=(1.5, 1.5, 1.5))
    r = X.exact_march((0, 0, -1.25), (0, 0, 1.0), tau=0.5, **args)
    assert r.absorbed and r.depth == F(1, 2) and r.cell == (0, 0, 0) and r.component == 0 and r.t0 == F(11, 4)
    r = X.exact_march((0, 0, -1.25), (0, 0, 1.0), tau=1.25, **args)      # 0.75 in cell 0, 0.5 more at rate 2
    assert r.absorbed and r.depth == F(3, 2) and r.cell == (0, 0, 2) and r.planes == 2
    r = X.exact_march((0, 0, -1.25), (0, 0, 1.0), tau=0.75 + 1.0 + 0.5, **args)   # exactly the whole chord: not before t0
    assert not r.absorbed and r.ambiguous
    r = X.exact_march((0, 0, 1.25), (0, 0, -1.0), tau=0.5, **args)       # downwards: 0.75 at rate 0.5 first
    assert r.absorbed and r.cell == (0, 0, 2) and r.depth == F(3, 4) + (F(1, 2) - F(3, 8)) / 2
    r = X.exact_march((0.25, 0, 0.0), (1.0, 0, 0), tau=0.5, **args)      # inside the plane z = 0: the cell above it
    assert r.absorbed and r.cell == (0, 0, 2) and r.depth == F(1, 4)
    two = dict(args, values=[vals[0], None], alphas=[1.0, 0.5])
    r = X.exact_march((0, 0, -0.25), (1.0, 0, 0), tau=0.25, **dict(two, u1=0.9))   # clear for the first: the second
    assert r.absorbed and r.cell == (0, 0, 1) and r.component == 1 and r.depth == F(1, 2)


def host_march(case, scene, block, pos, dirs, u0, u1, refs):
    """The host's decisions for every ray: (absorbed, depth, cell, component index)."""
    medium = block.geometry.material
    out = []
    draws = []
    uniform = np.random.uniform
    np.random.uniform = lambda *a, **k: draws.pop()
    try:
        for i in range(case.n):
            local = Ray(tuple(pos[i]), tuple(dirs[i]), case.wavelength).representation(scene.root, block)
            draws.append(float(u0[i]))
            absorbed, depth, cell = medium.is_absorbed_in(local, float(refs[i].t0))
            k = None
            if absorbed:
                draws.append(float(u1[i]))
                k = medium.components.index(medium.component_at(case.wavelength, cell))
            assert not draws
            out.append((bool(absorbed), float(depth), cell, k))
    finally:
        np.random.uniform = uniform
    return out


def judge(case, refs, got, who):
    """The checks of one case, shared with the GPU test: `got` per ray (absorbed, depth, cell or None, component).
    Returns the worst |depth - exact| / bound."""
    worst, worst_ulps, ambiguous = 0.0, 0.0, 0
    for i, (r, (absorbed, depth, cell, comp)) in enumerate(zip(refs, got)):
        if r.ambiguous:
            ambiguous += 1
            if absorbed != r.absorbed or (cell is not None and cell != r.cell):
                continue
        assert absorbed == r.absorbed, (who, case, i, "absorbed", absorbed, float(r.depth), float(r.t0))
        if not absorbed:
            continue
        if cell is not None:
            assert tuple(cell) == r.cell, (who, case, i, "cell", cell, r.cell)
        err = abs(F(depth) - r.depth)
        assert err <= r.bound, (who, case, i, "depth", depth, float(r.depth), float(err / r.bound))
        worst = max(worst, float(err / r.bound))
        worst_ulps = max(worst_ulps, float(err / (X.U * max(r.depth, r.t0))))
        if not r.ambiguous:
            assert comp == r.component, (who, case, i, "component", comp, r.component)
    print(f"{who} {case}: worst |depth - exact| / bound {worst:.3f}, {worst_ulps:.2f} ulp of max(depth, t0); "
          f"{ambiguous} ambiguous of {len(refs)}; {sum(r.absorbed for r in refs)} absorbed")
    if case.family == "A":
        assert ambiguous * 1000 <= len(refs), (who, case, ambiguous)
    else:
        assert ambiguous == 0, (who, case, ambiguous)
    return worst


@pytest.mark.parametrize("case", X.CASES, ids=[c.name for c in X.CASES])
def test_the_host_march_agrees_with_the_exact_reference_ray_by_ray(case):
    scene, block, compiled, node_id, pos, dirs, u0, u1 = case_inputs(case)
    taus = -np.log(1 - u0)   # (the host's own draw: `is_absorbed_in`)
    refs = X.references(case, compiled, node_id, pos, dirs, taus, u1)
    n_abs = sum(r.absorbed for r in refs)
    assert 0.15 * case.n < n_abs < 0.9 * case.n
    assert len({r.cell for r in refs if r.absorbed}) >= 2 or case.shape == (1, 1, 1)
    if len(case.coefficients) > 1:
        assert len({r.component for r in refs if r.absorbed}) == len(case.coefficients)
    if case.family == "B":   # the family holds what it is for: rays inside a plane, through edges and through vertices
        assert sum(r.in_plane for r in refs) > case.n // 20
        many = [n for n in case.shape if n > 1]
        if len(many) >= 2:
            assert sum(r.ties2 > 0 for r in refs) > case.n // 20
        if len(many) == 3:
            assert sum(r.ties3 > 0 for r in refs) > case.n // 100
    judge(case, refs, host_march(case, scene, block, pos, dirs, u0, u1, refs), "host")
