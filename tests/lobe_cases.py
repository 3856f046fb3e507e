"""Scattering coatings (`ScatterLobe`): the cases, a float64 restatement of the rule and an exact reference of it
(tests/test_coating_lobes.py, tests/test_gpu_coating_lobes.py).

`kernel_turn` restates rules 2-5 of the contract text in include/pvtrace_hip.h ("Scattering coatings") in float64, one
operation per operation of the text; `exact_turn` evaluates the same rules exactly: the outgoing normal and the axis in
mpmath from the exact values of the input doubles, the row pick and the CDF inversion by
`exact_events.exact_phase_turn` (rationals), the turn about the EXACT axis and the fold in mpmath.  Neither is written
from the kernel or from the host delegate.

The bound (U = 2^-53, first order in U, an ABSOLUTE error of each component of d'; the constants U, S_SQRT,
TRIG_KERNEL / TRIG_HOST and E_B are `exact_events`')
------------------------------------------------------------------------------------------------------------------
 1. The axis a.  "normal" (+-N) and "straight" (d) are input doubles: e_a = 0.  "specular", a = d - 2 (d.N) N: the dot
    product is three products and two sums of terms <= 1, e_dd = 3 U; each component adds the roundings of 2 dd N_c and
    of the difference: e_a = 2 e_dd + 3 U = 9 U.  "refracted" (the terms of `exact_coating` item 4 / `exact_events` item
    9 with an exact normal): n = fl(n1 / n2) (U n), dd = d.nf (e_dd = 3 U), x = 1 - n^2 (1 - dd^2):
    e_x = n^2 (2 dd e_dd + 2 U) + 6 U n^2 (1 - dd^2) + U; c = sqrt(x): e_c = rt(x, e_x) + S_SQRT U c; k = c - n dd:
    e_k = e_c + n e_dd + 3 U n dd + U |k|; a = n d + k nf: e_a = e_k + 4 U (n + |k|).
 2. The turn about a.  `PhaseExact.bound` (exact_events, "Phase turn", items 1-4) bounds the turn about an axis that is
    an exact double.  An axis off by e_a per component moves mu a by |mu| e_a and each basis component by at most
    5 e_a (e1, e2 are polynomials in x, y and a = -1 / (s + z), |a| <= 1: |d/dx| <= 2, |d/dy| <= 2, |d/dz| <= 1), so
    st (cos e1 + sin e2) by st sqrt(2) 5 e_a <= 8 st e_a:   B = PhaseExact.bound + (|mu| + 8 st) e_a.
    Where |a.z| <= e_a the sign s = copysign(1, a.z) of the basis is not decided: the ray is ambiguous.
 3. The fold.  t = d'.N_out with N_out exact: |t - exact| <= 3 B + 6 U =: e_t.  The mirror about the exact N_out keeps
    the 2-norm of the error vector (<= sqrt(3) B) and adds its own roundings: a folded ray, and one whose fold is
    ambiguous, has the bound 2 B + 9 U.
 4. 4 U of slack for the second-order terms.
A ray is AMBIGUOUS under the conditions of `exact_events.check_phase_conditions` (|u1 - t| within its bound: either
row is accepted), where |d'.N_out| <= e_t (either fold is accepted), or where |a.z| <= e_a.  A case may have at most 1 %
of ambiguous rays, counted in the references alone.

`kernel_turn` against the kernel: two float64 evaluations of the same rule, each within its own bound of the exact
value (TRIG_HOST for the restatement's numpy sine and cosine, TRIG_KERNEL for pvt_sincos2pi): `pair_bound` is the sum
of the two, evaluated in float64 from the restatement's own mu and axis.

The cases (each with incidence from both sides of a face of a rotated box of n = 1.5, or on a sphere covered by
`Coating(None, ...)`) are listed in CASES; FAULTS names the wrong rules every one of which must move at least 20 rays
of some case, in the references alone.
"""
import functools
import math

import numpy as np
from mpmath import mp, mpf

from pvtrace_amd import (
    Box, CoatedSurfaceDelegate, Coating, Material, Node, PhaseFunctionTable, ScatterLobe, Scene, Sphere, Surface,
)
from pvtrace_amd.engine import compile_scene
from pvtrace_amd.material import ray_basis
from tests import exact_events as X
from tests.exact_emission import stream

SEED = 7100          # ray i of a case draws from the stream SEED + i
N_RAYS = 1000
ME = 8               # max_events of every history launch
MAXSTEPS = 32
DRAWS = 6 * ME
GENERATE, REFLECT, TRANSMIT, EXIT = 0, 1, 2, 7
N_BOX = 1.5
SIZE = (40.0, 40.0, 2.0)
RADIUS = 2.0
ROT = X.ROT
U = float(X.U)
FAULTS = ("no-fold", "fold-about-N", "axis-not-flipped", "u1-always", "normal-as-fresnel")


def _two_row_table():
    angle = np.linspace(0.0, 180.0, 181)
    wide = np.where(angle < 90.0, np.cos(np.radians(angle)), 0.0)
    narrow = np.exp(-0.5 * (angle / 12.0) ** 2)
    return PhaseFunctionTable(angle, np.vstack([wide, narrow]), wavelength=[500.0, 600.0])


COSINE = ScatterLobe.lambertian()
COSINE_BIG = ScatterLobe.lambertian(nodes=4097)
TWO_ROW = _two_row_table()


class LobeCase:
    """One case: the coating of the node (every face of the box, or the whole sphere), the incidence of its rays."""

    def __init__(self, name, reflection="specular", transmission="fresnel", reflectivity=1.0, geometry="box",
                 incidence=(0.0, 75.0), wavelength=555.0):
        self.name, self.reflection, self.transmission = name, reflection, transmission
        self.reflectivity, self.geometry, self.incidence, self.wavelength = reflectivity, geometry, incidence, wavelength
        self.n = N_RAYS

    def __repr__(self):
        return self.name

    def coating(self, reflection=None, transmission=None):
        return Coating(None, reflectivity=self.reflectivity, reflection=reflection or self.reflection,
                       transmission=transmission or self.transmission)

    def scene(self, coating=None):
        """(scene, the coated node).  `coating`: another coating in place of the case's."""
        world = Node(name="world", geometry=Box((400.0, 400.0, 400.0), material=Material(refractive_index=1.0)))
        surface = Surface(delegate=CoatedSurfaceDelegate([coating or self.coating()]))
        material = Material(refractive_index=N_BOX, surface=surface)
        geometry = Box(SIZE, material=material) if self.geometry == "box" else Sphere(RADIUS, material=material)
        node = Node(name="lobe", parent=world, geometry=geometry)
        node.rotate(*ROT)
        node.translate((0.3, -0.7, 0.9))
        return Scene(world), node

    def matched_beyond(self):
        """Rule 1: beyond the critical angle the coating's R applies ("matched", a lobe about "normal" or "straight")."""
        t = self.transmission
        return t.about != "refracted" if isinstance(t, ScatterLobe) else t == "matched"

    def rays(self):
        """(positions, directions, wavelengths, inside, normals at the hit) in the world frame: even rays arrive from
        outside, odd rays from inside the node, at the case's angles of incidence (degrees, uniform between the two) and a
        uniform azimuth."""
        rng = np.random.default_rng(sum(map(ord, self.name)))
        n = self.n
        theta = np.radians(rng.uniform(self.incidence[0], self.incidence[1], n))
        phi = rng.uniform(0.0, 2.0 * np.pi, n)
        inside = np.arange(n) % 2 == 1
        if self.geometry == "box":
            p = np.column_stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), np.full(n, 0.5 * SIZE[2])])
            normal = np.tile([0.0, 0.0, 1.0], (n, 1))
        else:
            v = rng.normal(size=(n, 3))
            normal = v / np.linalg.norm(v, axis=1)[:, None]
            p = RADIUS * normal
        e1, e2 = ray_basis(normal)
        tangent = np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2
        sign = np.where(inside, 1.0, -1.0)[:, None]            # from inside the ray travels along the outward normal
        d = np.sin(theta)[:, None] * tangent + sign * np.cos(theta)[:, None] * normal
        if self.geometry == "box":
            back = np.where(inside, 0.5 * SIZE[2] / np.cos(theta), 3.0)
        else:
            back = np.where(inside, RADIUS * np.cos(theta), 3.0)
        start = p - back[:, None] * d
        scene, _ = self.scene()
        compiled = compile_scene(scene)
        m = np.asarray(compiled.local_to_world[compiled.node_names.index("lobe")], dtype=np.float64)
        pos = start @ m[:3, :3].T + m[:3, 3]
        dirs = d @ m[:3, :3].T
        dirs = dirs / np.linalg.norm(dirs, axis=1)[:, None]
        normals = normal @ m[:3, :3].T
        return pos, dirs, np.full(n, float(self.wavelength)), inside, normals


CASES = [
    LobeCase("cosine-reflection", reflection=COSINE),
    LobeCase("cosine-transmission", transmission=ScatterLobe(COSINE.table, "normal"), reflectivity=0.0),
    LobeCase("gloss-specular-20", reflection=ScatterLobe.gaussian(5.0, "specular"), incidence=(20.0, 20.0)),
    LobeCase("gloss-specular-80", reflection=ScatterLobe.gaussian(10.0, "specular"), incidence=(80.0, 80.0)),
    LobeCase("refracted-30", transmission=ScatterLobe.gaussian(5.0, "refracted"), reflectivity=0.0, incidence=(30.0, 30.0)),
    LobeCase("refracted-60", transmission=ScatterLobe.gaussian(5.0, "refracted"), reflectivity=0.0, incidence=(60.0, 60.0)),
    LobeCase("straight-30", transmission=ScatterLobe.gaussian(5.0, "straight"), reflectivity=0.0, incidence=(30.0, 30.0)),
    LobeCase("straight-60", transmission=ScatterLobe.gaussian(5.0, "straight"), reflectivity=0.0, incidence=(60.0, 60.0)),
    LobeCase("two-rows-between", reflection=ScatterLobe(TWO_ROW, "normal"), wavelength=550.0),
    LobeCase("cosine-4097", reflection=COSINE_BIG),
    LobeCase("sphere-both", reflection=COSINE, transmission=ScatterLobe(COSINE.table, "normal"), reflectivity=0.5,
             geometry="sphere", incidence=(0.0, 35.0)),
]
BY_NAME = {c.name: c for c in CASES}


# ---- the decision that precedes the turn (rule 1), in float64 ----------------------------------------------------------------
def outcome(case, d, normal, inside, draws, fault=None):
    """(kind, draws consumed, near): rule 1 for a photon arriving along `d` at a point of geometric `normal`, from inside
    the node (n = 1.5 -> 1) or from outside.  R is the coating's scalar, or 1 beyond the critical angle on a coating that
    does not behave as "matched" there; u is drawn when R > 0.  `near`: within 1e-9 of the critical cosine."""
    c1 = min(abs(float(np.dot(normal, d))), 1.0)
    r = float(case.reflectivity)
    near = False
    if inside:
        cc = math.sqrt(1.0 - (1.0 / N_BOX) ** 2)
        near = abs(c1 - cc) < 1e-9
        matched = case.matched_beyond()
        if fault == "normal-as-fresnel" and isinstance(case.transmission, ScatterLobe) and case.transmission.about == "normal":
            matched = False
        if c1 < cc and not matched:
            r = 1.0
    if r > 0.0:
        return (REFLECT if draws[0] < r else TRANSMIT), 1, near
    return TRANSMIT, 0, near


# ---- the float64 restatement of rules 2-5 --------------------------------------------------------------------------------------
def _axis(about, d, normal, s, n1, n2):
    """Rule 3 in float64: the axis of a lobe, or the direction of a built-in mode ("specular", "fresnel", "matched")."""
    if about in ("straight", "matched"):
        return np.array(d, dtype=np.float64)
    nf = -s * normal                           # the normal along the ray
    dd = float(nf[0] * d[0] + nf[1] * d[1] + nf[2] * d[2])
    if about == "specular":
        return np.array([d[c] - 2.0 * dd * nf[c] for c in range(3)])
    n = n1 / n2                                # "refracted" / "fresnel"
    c = math.sqrt(1.0 - n * n * (1.0 - dd * dd))
    sign = -1.0 if dd < 0.0 else 1.0
    k = sign * (c - sign * n * dd)
    return np.array([n * d[c_] + k * nf[c_] for c_ in range(3)])


def kernel_turn(mode, transmit, d, normal, wl, draws, n1=1.0, n2=1.0, fault=None):
    """Rules 2-5 in float64 -> (direction, draws consumed, (mu, mu_j, axis)).  `mode`: the slot's ScatterLobe or built-in
    string; `draws`: the stream behind u."""
    d = np.asarray(d, dtype=np.float64)
    normal = np.asarray(normal, dtype=np.float64)
    s = 1.0 if float(normal[0] * d[0] + normal[1] * d[1] + normal[2] * d[2]) < 0.0 else -1.0
    if not isinstance(mode, ScatterLobe):
        return _axis(mode, d, normal, s, n1, n2), 0, None
    so = -s if transmit else s
    if fault == "axis-not-flipped":
        so = s
    n_out = so * normal
    axis = n_out if mode.about == "normal" else _axis(mode.about, d, normal, s, n1, n2)
    table = mode.table
    at = 0
    u1 = 0.0
    if table.n_wavelength > 1 or fault == "u1-always":
        u1, at = draws[0], 1
    u2, u3 = draws[at], draws[at + 1]
    row = int(table.rows(wl, u1))
    mu = float(table.sample_mu(u2, row))
    j = min(int(np.searchsorted(table.cdf[row], u2, side="right")) - 1, table.mu.size - 2)
    st = math.sqrt((1.0 - mu) * (1.0 + mu))
    phi = 2.0 * math.pi * u3
    cp, sp = math.cos(phi), math.sin(phi)
    e1, e2 = ray_basis(axis)
    out = np.array([mu * axis[c] + st * (cp * e1[c] + sp * e2[c]) for c in range(3)])
    fold_n = normal if fault == "fold-about-N" else n_out
    t = (out[0] * fold_n[0] + out[1] * fold_n[1]) + out[2] * fold_n[2]
    if t < 0.0 and fault != "no-fold":
        out = np.array([out[c] - (2.0 * t) * fold_n[c] for c in range(3)])
    return out, at + 2, (mu, float(table.mu[j]), axis)


def axis_error(about, d, normal, n1, n2):
    """e_a of item 1 of the bound, in float64 (a bound: evaluated generously)."""
    if about in ("normal", "straight"):
        return 0.0
    if about == "specular":
        return 9.0 * U
    dd = min(abs(float(np.dot(normal, d))), 1.0)
    n = n1 / n2
    x = max(1.0 - n * n * (1.0 - dd * dd), 0.0)
    e_x = n * n * (2.0 * dd * 3.0 * U + 2.0 * U) + 6.0 * U * n * n * (1.0 - dd * dd) + U
    c = math.sqrt(x)
    e_c = (math.sqrt(e_x) if x == 0.0 else min(e_x / c, math.sqrt(e_x))) + X.S_SQRT * U * c
    k = abs(c - n * dd)
    e_k = e_c + n * 3.0 * U + 3.0 * U * n * dd + U * k
    return e_k + 4.0 * U * (n + k)


def turn_bound(mu, mu_j, e_a, trig):
    """B of item 2 (+ item 4) in float64 from the restatement's own mu: `PhaseExact.bound`'s expression, then the axis."""
    st = math.sqrt(max(0.0, 1.0 - mu * mu))
    e_mu = 4.0 * U * abs(mu - mu_j) + U * max(abs(mu), abs(mu_j))
    arg = max(0.0, 1.0 - mu * mu)
    e = 2.0 * abs(mu) * e_mu
    e_st = (math.sqrt(e) if arg == 0.0 else min(e / math.sqrt(arg), math.sqrt(e))) + 3.0 * U * st
    b = e_mu + 2.0 * U + 2.0 * e_st + st * (2 * trig + 2 * X.E_B + 3) * U + 4.0 * U
    return b + (abs(mu) + 8.0 * st) * e_a + 4.0 * U


def pair_bound(mode, d, normal, info, n1, n2):
    """The bound between `kernel_turn` and another float64 evaluation with the kernel's sine and cosine: the sum of the
    two bounds to the exact value, the fold's factor included (2 B + 9 U each), generously for every ray."""
    if info is None:   # a built-in mode: the axis itself
        e = axis_error({"specular": "specular", "fresnel": "refracted", "matched": "straight"}[mode], d, normal, n1, n2)
        return 2.0 * e + 8.0 * U
    mu, mu_j, _ = info
    e_a = axis_error(mode.about, d, normal, n1, n2)
    return sum(2.0 * turn_bound(mu, mu_j, e_a, trig) + 9.0 * U for trig in (X.TRIG_KERNEL, X.TRIG_HOST))


# ---- the exact reference -----------------------------------------------------------------------------------------------------
class LobeExact:
    """kind; candidates: [(direction (mpf), bound)] every one of which is accepted (one unless ambiguous); ambiguous;
    folded: the reference takes the fold; used: draws consumed by the turn; fold_margin."""
    __slots__ = ("kind", "candidates", "ambiguous", "folded", "used", "phase", "bound", "fold_margin")


@X.precise
def exact_turn(mode, transmit, d, normal, wl, draws, n1=1.0, n2=1.0, trig=X.TRIG_HOST):
    """Rules 2-5 exactly, on the exact values of the input doubles."""
    out = LobeExact()
    dd = [mpf(float(c)) for c in d]
    nn = [mpf(float(c)) for c in normal]
    s = 1 if X.dot(nn, dd) < 0 else -1
    so = -s if transmit else s
    n_out = [so * c for c in nn]
    about = mode.about
    e_a = mpf(axis_error(about, np.asarray(d, dtype=np.float64), np.asarray(normal, dtype=np.float64), n1, n2))
    if about == "normal":
        axis = n_out
    elif about == "straight":
        axis = dd
    else:
        nf = [-s * c for c in nn]
        dn = X.dot(dd, nf)
        if about == "specular":
            axis = [dd[c] - 2 * dn * nf[c] for c in range(3)]
        else:
            n = mpf(float(n1)) / mpf(float(n2))
            k = mp.sqrt(1 - n * n * (1 - dn * dn)) - n * dn
            axis = [n * dd[c] + k * nf[c] for c in range(3)]
    table = mode.table
    at = 1 if table.n_wavelength > 1 else 0
    u1 = draws[0] if at else 0.0
    u2, u3 = draws[at], draws[at + 1]
    axis_d = [float(c) for c in axis]
    ph = X.exact_phase_turn(table, wl, axis_d, u1, u2, u3, trig=trig)
    out.phase, out.used = ph, at + 2
    e1, e2 = X.duff_basis(axis[0], axis[1], axis[2], axis_d[2])
    phi = 2 * mp.pi * mpf(float(u3))
    cp, sp = mp.cos(phi), mp.sin(phi)
    out.candidates = []
    out.ambiguous = ph.ambiguous or (e_a > 0 and abs(axis[2]) <= e_a)
    out.folded, out.fold_margin = False, None
    for row, (j, mu_q, _, bound) in ph.rows.items():
        mu = mpf(mu_q.numerator) / mpf(mu_q.denominator)
        st = mp.sqrt(max(mpf(0), 1 - mu * mu))
        direction = [mu * axis[c] + st * (cp * e1[c] + sp * e2[c]) for c in range(3)]
        b = bound + (abs(mu) + 8 * st) * e_a + 4 * X.U
        t = X.dot(direction, n_out)
        e_t = 3 * b + 6 * X.U
        folded = [direction[c] - 2 * t * n_out[c] for c in range(3)]
        if row == ph.row:
            out.folded, out.fold_margin, out.bound = t < 0, abs(t), b
        if abs(t) <= e_t:
            out.ambiguous = True
            out.candidates += [(direction, 2 * b + 9 * X.U), (folded, 2 * b + 9 * X.U)]
        elif t < 0:
            out.candidates.append((folded, 2 * b + 9 * X.U))
        else:
            out.candidates.append((direction, b))
    return out


@X.precise
def ratio(direction, ref):
    """min over the accepted candidates of |direction - exact| / bound."""
    return min(float(X.component_error(direction, want) / bound) for want, bound in ref.candidates)


# ---- a case's inputs and references, computed once ----------------------------------------------------------------------------
class Inputs:
    pass


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The rays of a case, their draws, the first event's outcome by rule 1 and the mode that turns each ray."""
    case = BY_NAME[name]
    x = Inputs()
    x.case = case
    x.pos, x.dirs, x.wl, x.inside, x.normals = case.rays()
    x.draws = np.array([stream(SEED + i, DRAWS) for i in range(case.n)])
    x.kind, x.at, x.near = [], [], []
    for i in range(case.n):
        kind, used, near = outcome(case, x.dirs[i], x.normals[i], bool(x.inside[i]), x.draws[i])
        x.kind.append(kind)
        x.at.append(used)
        x.near.append(near)
    x.kind, x.at = np.array(x.kind), np.array(x.at)
    return x


def mode_of(case, kind):
    return case.transmission if kind == TRANSMIT else case.reflection


def indices(inside):
    """(n1, n2) of a photon that arrives from inside the node or from outside."""
    return (N_BOX, 1.0) if inside else (1.0, N_BOX)


@functools.lru_cache(maxsize=None)
def references(name, trig=X.TRIG_HOST):
    """Per ray the `LobeExact` of its first event, or None where a built-in mode turns it (total reflection on a
    "refracted" coating)."""
    x = inputs(name)
    refs = []
    for i in range(x.case.n):
        mode = mode_of(x.case, x.kind[i])
        if not isinstance(mode, ScatterLobe):
            refs.append(None)
            continue
        n1, n2 = indices(bool(x.inside[i]))
        refs.append(exact_turn(mode, x.kind[i] == TRANSMIT, x.dirs[i], x.normals[i], x.wl[i], list(x.draws[i][x.at[i]:]),
                               n1, n2, trig=trig))
    return refs


def restated(name, fault=None):
    """Per ray (kind, direction) of the first event by `outcome` and `kernel_turn`, under a named wrong rule if any."""
    x = inputs(name)
    got = []
    for i in range(x.case.n):
        inside = bool(x.inside[i])
        kind, used, _ = outcome(x.case, x.dirs[i], x.normals[i], inside, x.draws[i], fault=fault)
        n1, n2 = indices(inside)
        direction, _, _ = kernel_turn(mode_of(x.case, kind), kind == TRANSMIT, x.dirs[i], x.normals[i], x.wl[i],
                                      list(x.draws[i][used:]), n1, n2, fault=fault)
        got.append((kind, direction))
    return got
