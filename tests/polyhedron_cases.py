"""Cases shared by tests/test_polyhedron.py and tests/test_gpu_polyhedron.py: the convex polyhedra, their fixed-seed ray
families, and the EXACT reference the crossing distances of `pvtrace_amd.Polyhedron` are held to.

The reference takes the stored doubles of a case -- plane rows, ray origin and direction -- as rationals
(`fractions.Fraction`; every double is an integer multiple of 2^-1074, so the arithmetic is carried out on those integers)
and computes, for every plane k, den_k = n_k.d and num_k = h_k - n_k.o exactly, hence t_k = num_k / den_k exactly, the
entry distance tin = max { t_k : den_k < 0 } and the exit distance tout = min { t_k : den_k > 0 }.  The exact quotient is
rounded ONCE to a double for the comparisons (Python's int / int is correctly rounded): that rounding, u |t|, is added to
the bound below.

The bound B_k(t) of a computed plane distance, from the operation sequence of the class docstring (u = 2^-53):

  * den = (nx*dx + ny*dy) + nz*dz: every term passes through at most three roundings (its product and two sums), so
    |d den| <= 3u D with D = |nx dx| + |ny dy| + |nz dz|.
  * num = h - ((nx*ox + ny*oy) + nz*oz): three roundings on the dot product, 3u O with O = |nx ox| + |ny oy| + |nz oz|,
    and one on the subtraction, u (|h| + O): |d num| <= 4u (|h| + O).
  * t = num / den: one rounding, u |t|.
  * First order: |dt| <= (|d num| + |t| |d den|) / |den| + u |t|.  A ray is only judged when |den| > 8u D (below), so
    the relative error of den is below 3/8 and the neglected factor 1 / (1 - 3/8) = 1.6 -- with the products of the
    small terms -- is covered by DOUBLING the first-order sum:
        B_k(t) = 2 ((4u (|h| + O) + 3u D |t|) / |den| + u |t|) + u |t|      (the last term: the reference's own rounding).
  * An extremum.  The doubles' tin is the computed distance of SOME plane m; it is at least the computed distance of the
    exact maximiser k*, hence >= tin - B_k*, and at most t_m + B_m <= tin + B_m.  Plane m can only be one whose interval
    reaches the best lower end: t_m + B_m >= max_j (t_j - B_j).  So B(tin) = max of B_k over those contenders; likewise
    for tout with min.

A ray is AMBIGUOUS when the reference cannot say what doubles should do:

  * a `den` whose sign lies within its error: 0 < |den| <= 8u D, or |den| within a factor two of the 1e-300 threshold;
    a plane with D == 0 (every product an exact zero: doubles compute den == 0 as well) is parallel for both, and then
    a `num` within 4u (|h| + O) of zero is ambiguous, since its sign decides the miss;
  * tin and tout closer than B(tin) + B(tout): a graze of an edge or a vertex;
  * a candidate within its B of EPS_ZERO.

A family may hold at most 2 % of such rays (`MAX_AMBIGUOUS`, the project's cap).
"""
import functools
import math
from fractions import Fraction as Fr

import numpy as np

from pvtrace_amd.geometry import EPS_ZERO, Polyhedron

U = 2.0 ** -53
INFLATE = 1.0 + 1e-9          # the bounds themselves are evaluated in doubles: rounded up by far more than their own error
MAX_AMBIGUOUS = 0.02
N_RAYS = 300
_ONE = 2 ** 1074              # 2^1074 x is an integer for every double x
_ONE2 = _ONE * _ONE

WEDGE = ((-1.0, -0.25), (1.0, -0.05), (1.0, 0.05), (-1.0, 0.25))
TETRA = 0.8 * np.array([(1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0)])
PYRAMID = np.array([(sx * r, sy * r, z) for z, r in ((-0.5, 1.0), (0.5, 0.4)) for sx in (-1.0, 1.0) for sy in (-1.0, 1.0)])

SHAPES = ("hexagon", "triangle", "wedge", "tetra", "pyramid", "needle", "round")
FAMILIES = ("outside", "inside", "edges", "vertices", "parallel")
# a node's pose in the world of the GPU cases: None, or (angle, axis, translation)
POSES = {"own": None, "posed": (0.7, (1.0, 2.0, 3.0), (0.3, -0.2, 0.5))}


@functools.lru_cache(maxsize=None)
def shape(name):
    """The polyhedron of a name (no material), built once."""
    if name == "hexagon":
        return Polyhedron.regular_prism(6, 1.0, 0.4)
    if name == "triangle":
        return Polyhedron.regular_prism(3, 1.0, 0.5, phase=0.3)
    if name == "wedge":
        return Polyhedron.prism(WEDGE, 1.5)
    if name == "tetra":
        return Polyhedron.from_vertices(TETRA)
    if name == "pyramid":
        return Polyhedron.from_vertices(PYRAMID)
    if name == "needle":
        return Polyhedron.regular_prism(5, 0.05, 10.0)
    if name == "round":
        return Polyhedron.regular_prism(62, 1.0, 0.4)
    raise KeyError(name)


def parallel_axes(name):
    """The axes a for which some plane's normal has an exactly zero a-component."""
    n = shape(name).planes[:, :3]
    return [a for a in range(3) if np.any(n[:, a] == 0.0)]


def families_of(name):
    return [f for f in FAMILIES if f != "parallel" or parallel_axes(name)]


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt(np.sum(v * v, axis=-1, keepdims=True))


def _isotropic(rng, n):
    z = rng.uniform(-1.0, 1.0, n)
    phi = rng.uniform(0.0, 2.0 * math.pi, n)
    s = np.sqrt(1.0 - z * z)
    return np.column_stack((s * np.cos(phi), s * np.sin(phi), z))


def _inside_points(rng, n, vertices, fill=0.9):
    """Random convex combinations of the vertices, drawn towards the centroid by `fill`."""
    w = rng.dirichlet(np.ones(len(vertices)), n) if len(vertices) <= 16 else rng.dirichlet(np.full(len(vertices), 0.05), n)
    centre = vertices.mean(axis=0)
    return centre + fill * (w @ vertices - centre)


def _towards(rng, targets, centre, R, inside_points):
    """Rays aimed at `targets`: from a sphere of radius 3R, or (every other ray) from `inside_points`."""
    n = len(targets)
    origins = centre + 3.0 * R * _isotropic(rng, n)
    if inside_points is not None:
        origins[1::2] = inside_points[1::2]
    return origins, _unit(targets - origins)


def rays(name, family):
    """(origins, directions), (N_RAYS, 3) each, in the shape's own frame: fixed seed per (shape, family)."""
    solid = shape(name)
    vertices = solid.vertices
    centre = vertices.mean(axis=0)
    R = float(np.max(np.sqrt(np.sum((vertices - centre) ** 2, axis=1))))
    lo, hi = vertices.min(axis=0), vertices.max(axis=0)
    rng = np.random.default_rng(1000 * SHAPES.index(name) + FAMILIES.index(family))
    n = N_RAYS
    if family == "outside":     # generic rays from outside, aimed into the bounding box
        return _towards(rng, rng.uniform(lo, hi, (n, 3)), centre, R, None)
    if family == "inside":      # generic rays from inside
        return _inside_points(rng, n, vertices), _isotropic(rng, n)
    if family in ("edges", "vertices"):   # at a point of an edge / a vertex displaced by 1e-1 .. 1e-12 of the size, half from inside
        if family == "edges":
            edges = sorted({(min(a, b), max(a, b)) for loop in solid.faces for a, b in zip(loop, loop[1:] + loop[:1])})
            pick = rng.integers(0, len(edges), n)
            s = rng.uniform(0.0, 1.0, n)[:, None]
            ends = np.array(edges)[pick]
            target = (1.0 - s) * vertices[ends[:, 0]] + s * vertices[ends[:, 1]]
        else:
            target = vertices[rng.integers(0, len(vertices), n)]
        target = target + _isotropic(rng, n) * (R * 10.0 ** -rng.uniform(1.0, 12.0, n))[:, None]
        return _towards(rng, target, centre, R, _inside_points(rng, n, vertices))
    if family == "parallel":    # along +-e_a where a plane's normal has an exactly zero a-component; origins inside and outside
        axes = parallel_axes(name)
        a = np.array(axes)[rng.integers(0, len(axes), n)]
        d = np.zeros((n, 3))
        d[np.arange(n), a] = np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
        o = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (n, 3))
        o[::2] = _inside_points(rng, n, vertices, fill=1.0)[::2]
        o = o - 3.0 * R * d * (rng.integers(0, 2, n) == 1)[:, None]   # (half of them start behind the solid)
        return o, d
    raise KeyError(family)


# ---- the exact reference -----------------------------------------------------------------------------------------------
def _int(x):
    """2^1074 x, exactly."""
    num, den = float(x).as_integer_ratio()
    return num * (_ONE // den)


@functools.lru_cache(maxsize=None)
def _int_rows(key):
    rows = np.frombuffer(key, dtype=np.float64).reshape(-1, 4)
    return [tuple(_int(v) for v in row) for row in rows], [tuple(float(v) for v in row) for row in rows]


class Crossing:
    __slots__ = ("t", "bound", "surface")

    def __init__(self, t, bound, surface):
        self.t, self.bound, self.surface = t, bound, surface


def plane_distances(planes, o, d):
    """Per plane of the (P, 4) double rows `planes`, for the ray (o, d) of doubles: ('parallel', num, err), ('unsure',) or
    (sense, t, B) with sense -1 (entry: den < 0) or +1 (exit), t the exact distance rounded once, B its bound."""
    irows, frows = _int_rows(np.ascontiguousarray(planes, dtype=np.float64).tobytes())
    fo, fd = [float(v) for v in o], [float(v) for v in d]
    io, id_ = [_int(v) for v in fo], [_int(v) for v in fd]
    out = []
    for (inx, iny, inz, ih), (nx, ny, nz, h) in zip(irows, frows):
        den = inx * id_[0] + iny * id_[1] + inz * id_[2]                  # 2^2148 n.d
        num = ih * _ONE - (inx * io[0] + iny * io[1] + inz * io[2])         # 2^2148 (h - n.o)
        D = abs(nx * fd[0]) + abs(ny * fd[1]) + abs(nz * fd[2])
        N = abs(h) + (abs(nx * fo[0]) + abs(ny * fo[1]) + abs(nz * fo[2]))
        if D == 0.0:
            if den != 0:
                out.append(("unsure",))
            else:
                out.append(("parallel", num / _ONE2, 4.0 * U * N * INFLATE))
            continue
        denf = abs(den / _ONE2)
        if denf <= 8.0 * U * D * INFLATE or denf < 2e-300:
            out.append(("unsure",))
            continue
        t = num / den
        B = (2.0 * ((4.0 * U * N + 3.0 * U * D * abs(t)) / denf + U * abs(t)) + U * abs(t)) * INFLATE
        out.append((-1 if den < 0 else 1, t, B))
    return out


def exact_crossings(planes, o, d):
    """(crossings, ambiguous) of the ray (o, d), doubles, with the exact solid of the double rows `planes`: the `Crossing`s
    in fold order -- entry, then exit -- and whether doubles may legitimately differ."""
    entries, exits, miss = [], [], False
    for k, item in enumerate(plane_distances(planes, o, d)):
        if item[0] == "unsure":
            return [], True
        if item[0] == "parallel":
            _, num, err = item
            if abs(num) <= err:
                return [], True
            miss = miss or num < 0.0
        else:
            (entries if item[0] < 0 else exits).append((item[1], item[2], k))
    if miss:
        return [], False

    def extremum(items, sign):   # sign +1: the maximum
        if not items:
            return -sign * math.inf, 0.0, -1
        best = max(sign * t - B for t, B, _ in items)
        bound = max(B for t, B, _ in items if sign * t + B >= best)
        t, _, k = max(items, key=lambda it: sign * it[0])
        return t, bound, k

    tin, b_in, k_in = extremum(entries, 1.0)
    tout, b_out, k_out = extremum(exits, -1.0)
    if abs(tout - tin) <= b_in + b_out:
        return [], True            # a graze of an edge or a vertex
    if tout < tin:
        return [], False
    found = []
    for t, bound, k in ((tin, b_in, k_in), (tout, b_out, k_out)):
        if not math.isfinite(t):
            continue
        if abs(t - EPS_ZERO) <= bound:
            return [], True
        if t > EPS_ZERO:
            found.append(Crossing(t, bound, k))
    return found, False


def judge(planes, o, d, distances):
    """`distances` (what the code under test found for the ray, in the order it found them) against the exact set ->
    (verdict, worst): verdict 'ambiguous', 'ok' or a string that says what is wrong; worst = max |t - t_exact| / B."""
    exact, ambiguous = exact_crossings(planes, o, d)
    if ambiguous:
        return "ambiguous", 0.0
    got = [float(t) for t in distances]
    if len(got) != len(exact):
        return f"{len(got)} crossings, the exact set has {len(exact)} ({[c.t for c in exact]} vs {got})", 0.0
    worst = 0.0
    for t, cr in zip(got, exact):
        err = abs(Fr(t) - Fr(cr.t))
        if err > Fr(cr.bound):
            return f"t = {t!r} on plane {cr.surface}: off the exact {cr.t!r} by {float(err):.3e} > B = {cr.bound:.3e}", 0.0
        worst = max(worst, float(err) / cr.bound)
    return "ok", worst


# ---- a node's pose, as the device applies it --------------------------------------------------------------------------
def to_local(w2l, pos, direction):
    """World ray -> node frame with the kernel's operation order: ((m0*x + m1*y) + m2*z) + t per row."""
    m = np.asarray(w2l, dtype=np.float64)
    o = np.array([((m[r, 0] * pos[0] + m[r, 1] * pos[1]) + m[r, 2] * pos[2]) + m[r, 3] for r in range(3)])
    d = np.array([(m[r, 0] * direction[0] + m[r, 1] * direction[1]) + m[r, 2] * direction[2] for r in range(3)])
    return o, d


def rotate(m, v):
    m = np.asarray(m, dtype=np.float64)
    return np.array([(m[r, 0] * v[0] + m[r, 1] * v[1]) + m[r, 2] * v[2] for r in range(3)])


# ---- the two closed-form laws (tests/test_gpu_polyhedron.py) ---------------------------------------------------------
LAW_SOURCE = (0.2, -0.1, 0.05)


def solid_angle_fractions(solid, source):
    """Per face of `solid`, the share of the full sphere it subtends from the interior point `source`: the sum over a fan
    of triangles of the face's loop (Van Oosterom and Strackee 1983), exact up to rounding."""
    v, p = solid.vertices, np.asarray(source, dtype=np.float64)
    out = []
    for loop in solid.faces:
        omega = 0.0
        a = v[loop[0]] - p
        for i, j in zip(loop[1:-1], loop[2:]):
            b, c = v[i] - p, v[j] - p
            la, lb, lc = (math.sqrt(float(np.dot(x, x))) for x in (a, b, c))
            num = float(np.dot(a, np.cross(b, c)))
            den = la * lb * lc + float(np.dot(a, b)) * lc + float(np.dot(a, c)) * lb + float(np.dot(b, c)) * la
            omega += 2.0 * math.atan2(abs(num), den)
        out.append(omega / (4.0 * math.pi))
    return out


def point_source_rays(n, seed=41):
    rng = np.random.default_rng(seed)
    return np.tile(LAW_SOURCE, (n, 1)), _isotropic(rng, n)


def chord_rays(n, seed=43, radius=2.0):
    """Uniform isotropic illumination: starts uniform on a sphere about the shape, directions by the cosine law about the
    inward normal."""
    rng = np.random.default_rng(seed)
    out = _isotropic(rng, n)
    ct = np.sqrt(rng.uniform(0.0, 1.0, n))
    st, phi = np.sqrt(1.0 - ct * ct), rng.uniform(0.0, 2.0 * math.pi, n)
    helper = np.where(np.abs(out[:, [2]]) < 0.9, np.array([[0.0, 0.0, 1.0]]), np.array([[1.0, 0.0, 0.0]]))
    e1 = _unit(np.cross(helper, out))
    e2 = np.cross(out, e1)
    d = -ct[:, None] * out + st[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    return radius * out, _unit(d)
