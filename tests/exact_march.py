"""An exact reference of the concentration-field march, and the ray families that hold the host march and the kernel
to it ray by ray (tests/test_field_march_exact.py, tests/test_gpu_field_march_exact.py).

The reference (`exact_march`) is written from the contract text of include/pvtrace_hip.h (PvtFieldTables, items 1-5),
in `fractions.Fraction` throughout, every input taken as the exact rational of its float64 value.  It does not walk
cells.  It forms the exact local ray p = R x + t, d = R v from the node's compiled world_to_local, the exact exit t0
from the container's box, and every interior plane crossing in (0, t0); it takes the cell of each open segment from
the segment's midpoint, accumulates alpha_cell * length, and solves tau(s) = tau* for s.  Two things are the
contract's DOUBLES, not rationals: the cell widths h = fl((upper - lower) / n) and the planes fl(lower + fl(i h)) --
with the true rational planes a ray inside a plane or through a vertex would disagree with a correct march.  A point
lies in the cell that counts the interior planes at or below it; the starting cell is also formed by the contract's
rule clamp(floor((p - lower) / h), 0, n - 1) on exact rationals, and a ray on which the two differ (a start within
the rounding of a plane) is marked ambiguous.

The tolerance (u = 2^-53; `Exact.bound`, a bound on |depth - exact depth| of a march given the same tau* bits)
-----------------------------------------------------------------------------------------------------------
The march evaluates depth = s_in + (tau* - tau_in) / alpha_cell with tau_in = sum_j alpha_j (s_j+1 - s_j) over the J
cells passed, s_i the parameters of the planes crossed.  To first order in u:

 1. Local transform.  p_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a: three products and three sums, so
    |dp_a| <= 3 u (sum_c |R_ac x_c| + |t_a|), and |dd_a| <= 3 u sum_c |R_ac v_c| for the direction.
 2. One division per plane crossed.  s_i = fl(fl(plane - p_a) / d_a): two roundings, and the errors of p_a and d_a
    divided by |d_a|:  e_i <= (dp_a + s_i dd_a) / |d_a| + 3 u s_i  (the third u: the plane's own distance from p).
 3. One multiply-add into tau_in per cell.  fl(alpha_j fl(s_out - s)) added to the running depth: u for the difference,
    u for the product, u tau_in for each of the J sums; alpha_j itself is a sum of C products in doubles, (C + 1) u.
    The plane errors enter tau_in telescoped, sum_i |alpha_before_i - alpha_after_i| e_i =: E.  Together
    |d tau_in| <= (J + C + 3) u tau_in + E.
 4. The final division.  fl(tau* - tau_in) (u), alpha_cell ((C + 1) u), the quotient (u), the sum with s_in (u depth):
    (C + 3) u (depth - s_in) + u depth, and s_in carries the error e_in of its own plane.

    bound = e_in + ((J + C + 3) u tau_in + E) / alpha_cell + (C + 3) u (depth - s_in) + u depth + 4 u max(depth, t0)

(the last term: slack for the second-order terms and for the host's fl(t0)).  In the issue's terms: a few ulps of
max(depth, t0), scaled by (1 + planes crossed) and by tau_in / alpha_cell = sum alpha_prev Delta / alpha_cell where a
dense cell precedes a thin one; the 1 / |d_a| of item 2 is what a rotated node adds for a ray nearly parallel to a
plane it crosses.  In an unrotated node with a dyadic translation and representable planes (family B) dp = dd = 0.

The same expression, evaluated with the alpha, tau_in and planes of any segment j, bounds the march's error of "where
would tau* be reached in segment j", the number it compares with the segment's end.  A ray is AMBIGUOUS when in some
segment that number lies within the segment's bound of the segment's end (at t0: the bound plus the error of the
tracer's own t0, taken as 4 e of item 2 for the exit plane, the mesh's triangle test included), or when u1 alpha_cell
lies within (2 C + 1) u alpha_cell of a partial sum (C products, C sums and the product u1 alpha_cell).  Ambiguous
rays are exempt from the equality of cell, component and absorbed-or-not, nothing else.

Position: the tracer advances x_c + v_c * adv in doubles, so a coordinate of the ABSORB row lies within
|v_c| bound + u |v_c adv| + u |x_c + v_c adv| of x + v depth.
"""
import functools
import math
from fractions import Fraction as F

import numpy as np

from pvtrace_amd import Absorber, Box, ConcentrationGrid, Material, Mesh, Node, Reactor, Scene, Surface
from pvtrace_amd.material import NullSurfaceDelegate

U = F(1, 2 ** 53)


class Exact:
    """What `exact_march` returns.  absorbed; depth (Fraction; t0 when not absorbed); cell (ix, iy, iz) or None;
    component (index in the node's order) or None; depth_margin: the least distance in s by which a segment's end was
    missed (passed or not reached); pick_margin: the distance of u1 alpha_cell to the nearest partial sum; bound: the
    tolerance on the depth (docstring above); ambiguous; t0; planes: distinct plane parameters passed before the depth;
    ties2, ties3: how many of them two / three axes share; in_plane: an axis the ray does not move along sits on a plane."""
    __slots__ = ("absorbed", "depth", "cell", "component", "depth_margin", "pick_margin", "bound", "pick_bound",
                 "ambiguous", "t0", "planes", "alpha_cell", "ties2", "ties3", "in_plane")


def lattice_planes(lower, upper, shape):
    """(h, planes) per axis: the contract's doubles h = fl((upper - lower) / n) and fl(lower + fl(i h)), i = 1 .. n - 1."""
    hs, planes = [], []
    for a in range(3):
        lo, hi, n = float(lower[a]), float(upper[a]), int(shape[a])
        h = (hi - lo) / float(n)
        hs.append(h)
        planes.append([lo + float(i) * h for i in range(1, n)])
    return hs, planes


def exact_march(pos, direction, w2l, lower, upper, shape, values, alphas, tau, u1, half):
    """The contract on exact rationals.  pos, direction: the world ray (float64); w2l: the node's compiled 4 x 4
    world_to_local; lower, upper, shape: the lattice; values: per component its (nx, ny, nz) array, None = no field
    (c = 1); alphas: alpha_k(lambda) per component; tau: tau* (float64); u1: the pick's uniform; half: the container
    box's half extents in the node's frame (its planes are -half and +half)."""
    R = [[F(float(w2l[a][c])) for c in range(3)] for a in range(3)]
    T = [F(float(w2l[a][3])) for a in range(3)]
    x = [F(float(v)) for v in pos]
    v = [F(float(c)) for c in direction]
    p = [R[a][0] * x[0] + R[a][1] * x[1] + R[a][2] * x[2] + T[a] for a in range(3)]
    d = [R[a][0] * v[0] + R[a][1] * v[1] + R[a][2] * v[2] for a in range(3)]
    dp = [3 * U * (sum(abs(R[a][c] * x[c]) for c in range(3)) + abs(T[a])) for a in range(3)]
    dd = [3 * U * sum(abs(R[a][c] * v[c]) for c in range(3)) for a in range(3)]
    C = len(alphas)

    def plane_error(a, s):
        return (dp[a] + s * dd[a]) / abs(d[a]) + 3 * U * s

    # t0: the exact exit from the container's box
    t0, exit_axis = None, None
    for a in range(3):
        if d[a] != 0:
            t = ((F(float(half[a])) if d[a] > 0 else -F(float(half[a]))) - p[a]) / d[a]
            if t0 is None or t < t0:
                t0, exit_axis = t, a
    assert all(abs(p[a]) < F(float(half[a])) for a in range(3)), "the ray does not start inside its container"
    e_t0 = 4 * plane_error(exit_axis, t0)

    hs, planes = lattice_planes(lower, upper, shape)
    fplanes = [[F(q) for q in planes[a]] for a in range(3)]

    def cell_of(point):
        return tuple(sum(1 for q in fplanes[a] if q <= point[a]) for a in range(3))

    out = Exact()
    start_by_rule = tuple(min(max(math.floor((p[a] - F(float(lower[a]))) / F(hs[a])), 0), int(shape[a]) - 1)
                          for a in range(3))
    out.ambiguous = start_by_rule != cell_of(p)

    crossings, axes = {}, {}   # s -> the largest error of a plane parameter that ties there; the axes that tie there
    out.in_plane = any(d[a] == 0 and p[a] in fplanes[a] for a in range(3))
    for a in range(3):
        if d[a] == 0:
            continue
        for q in fplanes[a]:
            s = (q - p[a]) / d[a]
            if 0 < s < t0:
                crossings[s] = max(crossings.get(s, 0), plane_error(a, s))
                axes[s] = axes.get(s, 0) + 1
    knots = sorted(crossings)
    ends = knots + [t0]
    ftau = F(float(tau))
    fal = [F(float(a_k)) for a_k in alphas]

    def coefficients(cell):
        return [fal[k] * (F(float(values[k][cell])) if values[k] is not None else 1) for k in range(C)]

    s_in, tau_in, e_in, E, alpha_prev = F(0), F(0), F(0), F(0), None
    margin = None
    out.absorbed, out.depth, out.cell, out.component, out.pick_margin = False, t0, None, None, None
    out.bound, out.pick_bound, out.planes, out.alpha_cell = 4 * U * t0, None, len(knots), None
    for j, s_out in enumerate(ends):
        mid = (s_in + s_out) / 2
        cell = cell_of([p[a] + mid * d[a] for a in range(3)])
        terms = coefficients(cell)
        ac = sum(terms)
        if alpha_prev is not None:
            E += abs(alpha_prev - ac) * e_in
        alpha_prev = ac
        if ac > 0:
            depth = s_in + (ftau - tau_in) / ac
            bound = (e_in + ((j + C + 3) * U * tau_in + E) / ac + (C + 3) * U * (depth - s_in) + U * depth
                     + 4 * U * max(depth, t0))
            e_out = e_t0 if j == len(knots) else crossings[s_out]
            miss = abs(depth - s_out)
            margin = miss if margin is None else min(margin, miss)
            if miss <= bound + e_out:
                out.ambiguous = True
            if depth < s_out:
                out.absorbed, out.depth, out.cell, out.bound, out.planes, out.alpha_cell = True, depth, cell, bound, j, ac
                target, running, sums = F(float(u1)) * ac, F(0), []
                for k in range(C):
                    running += terms[k]
                    sums.append(running)
                    if out.component is None and target <= running:
                        out.component = k
                out.pick_margin = min(abs(target - q) for q in sums)
                out.pick_bound = (2 * C + 1) * U * ac
                if C > 1 and out.pick_margin <= out.pick_bound:
                    out.ambiguous = True
                break
            tau_in += ac * (s_out - s_in)
        if j < len(knots):
            s_in, e_in = s_out, crossings[s_out]
    out.depth_margin = margin
    out.t0 = t0
    passed = [axes[s] for s in knots[:out.planes]]
    out.ties2, out.ties3 = passed.count(2), passed.count(3)
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------
ROT = (0.7, (0.3, -1.0, 0.6))
SPECTRUM = np.column_stack([[384.0, 512.0, 640.0, 768.0], [2.0, 1.25, 0.5, 0.25]])   # (every lookup below is exact)


def spectral_alpha(wavelength):
    """alpha(wavelength) of SPECTRUM as an exact rational (piecewise linear, clamped)."""
    xs, ys = SPECTRUM[:, 0], SPECTRUM[:, 1]
    if wavelength <= xs[0]:
        return F(ys[0])
    if wavelength >= xs[-1]:
        return F(ys[-1])
    lo = int(np.searchsorted(xs, wavelength, side="right")) - 1
    t = (F(wavelength) - F(xs[lo])) / (F(xs[lo + 1]) - F(xs[lo]))
    return F(ys[lo]) + t * (F(ys[lo + 1]) - F(ys[lo]))


class Case:
    """One lattice, its components, the node's placement and container, and the rays of its family."""

    def __init__(self, name, family, shape, coefficients, container="box", rotate=None, location=None,
                 wavelength=555.0, seed=1, n=1500):
        self.name, self.family, self.shape, self.container = name, family, tuple(shape), container
        self.coefficients = coefficients   # per component: (coefficient, "field" | "plain")
        self.rotate, self.location, self.wavelength, self.seed, self.n = rotate, location, wavelength, seed, n
        if family == "A":
            self.size = (2.0, 2.0, 2.0)
            self.lower, self.upper = (-0.7, -0.85, -0.45), (0.9, 0.6, 0.8)
        else:
            self.size = (3.0, 3.0, 3.0)
            self.lower, self.upper = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
        self.half = tuple(0.5 * s for s in self.size)

    def __repr__(self):
        return self.name

    @functools.cached_property
    def fields(self):
        """Per component its values (None: unfielded).  Family A: random, about a third of the cells zero (a shared
        fifth clear for every component), one cell 1e-280; family B: checkerboards, each component on its own squares."""
        rng = np.random.default_rng(1000 + self.seed)
        ix, iy, iz = np.indices(self.shape)
        out = []
        shared = rng.uniform(size=self.shape) < 0.2
        for k, (_, kind) in enumerate(self.coefficients):
            if kind != "field":
                out.append(None)
            elif self.family == "A":
                vals = rng.uniform(0.1, 2.0, self.shape)
                vals[shared | (rng.uniform(size=self.shape) < 0.15)] = 0.0
                flat = vals.reshape(-1)
                flat[(7 + 5 * k) % flat.size] = 1e-280
                out.append(vals)
            else:
                on = [(ix + iy + iz) % 2 == 0, (ix + iy + iz) % 2 == 1, (ix + iz) % 2 == 0][k % 3]
                out.append(np.where(on, [0.875, 0.375, 0.625][k % 3], 0.0))
        return out

    def components(self, fielded=True):
        comps = []
        for k, (coef, kind) in enumerate(self.coefficients):
            grid = None
            if fielded and kind == "field":
                grid = ConcentrationGrid(self.fields[k], self.lower, self.upper)
            cls = Reactor if k % 2 else Absorber
            comps.append(cls(coef if isinstance(coef, np.ndarray) else float(coef), concentration=grid, name=f"c{k}"))
        return comps

    def scene(self, fielded=True):
        """(scene, the fielded node).  "box": the analytic box in a world; "tile": the middle tile of a 6 x 6 array (37
        nodes: the kernel's node grid); "mesh": the box as 12 triangles."""
        world = Node(name="world", geometry=Box((64.0, 64.0, 64.0), material=Material(refractive_index=1.0)))
        material = Material(refractive_index=1.0, surface=Surface(NullSurfaceDelegate()),
                            components=self.components(fielded))
        geometry = Mesh.box(self.size, material=material) if self.container == "mesh" else Box(self.size, material=material)
        if self.container == "tile":
            block = None
            for i in range(36):
                row, col = divmod(i, 6)
                mine = i == 21
                g = geometry if mine else Box(self.size, material=Material(refractive_index=1.5,
                                                                          components=[Absorber(0.25, name=f"t{i}")]))
                tile = Node(name=f"tile-{row}-{col}", parent=world, geometry=g)
                tile.location = ((col - 2.5) * 4.0, (row - 2.5) * 4.0, 0.0)
                block = tile if mine else block
        else:
            block = Node(name="block", parent=world, geometry=geometry)
            if self.rotate is not None:
                block.rotate(*self.rotate)
            if self.location is not None:
                block.translate(self.location)
        return Scene(world), block

    def alphas(self):
        """alpha_k(wavelength), float64: scalars as given, SPECTRUM by its exact lookup (representable)."""
        out = []
        for coef, _ in self.coefficients:
            a = spectral_alpha(self.wavelength) if isinstance(coef, np.ndarray) else F(float(coef))
            assert F(float(a)) == a
            out.append(float(a))
        return out

    def local_rays(self):
        """(positions, directions) in the node's frame, before the node's placement."""
        rng = np.random.default_rng(self.seed)
        n = self.n
        if self.family == "A":
            pos = rng.uniform(-1.0, 1.0, (n, 3)) * (np.array(self.half) * (1.0 - 1e-6))
            v = rng.normal(size=(n, 3))
            return pos, v / np.linalg.norm(v, axis=1)[:, None]
        # B: every ray is aimed through a point L whose coordinates are multiples of 1 / 4 (which hold every plane of
        # the shapes 1, 2, 4, 8 on [-1, 1]: L lies on planes, edges, vertices, outer faces or outside the lattice) or,
        # one time in three, odd multiples of 1 / 16; it starts on L or up to three quarter steps before it on the axes
        # it moves along.  Directions: the axes, the face diagonals and the body diagonals, both signs, equal
        # components bit-equal, so the plane parameters of different axes tie exactly.
        r2, r3 = 1.0 / math.sqrt(2.0), 1.0 / math.sqrt(3.0)
        dirs = []
        for a in range(3):
            for s in (1.0, -1.0):
                e = [0.0, 0.0, 0.0]
                e[a] = s
                dirs.append(e)
            b, c = (a + 1) % 3, (a + 2) % 3
            for sb in (r2, -r2):
                for sc in (r2, -r2):
                    e = [0.0, 0.0, 0.0]
                    e[b], e[c] = sb, sc
                    dirs.append(e)
        for sx in (r3, -r3):
            for sy in (r3, -r3):
                for sz in (r3, -r3):
                    dirs.append([sx, sy, sz])
        dirs = np.array(dirs)
        dirs = dirs[np.arange(n) % len(dirs)]
        quarter = rng.integers(-5, 6, (n, 3)) * 0.25
        off = (2 * rng.integers(-11, 11, (n, 3)) + 1) * 0.0625
        through = np.where(rng.uniform(size=(n, 3)) < 0.67, quarter, off)
        for a in range(3):   # (half of the time an interior plane of this very lattice, where it has one)
            if self.shape[a] > 1:
                planes = -1.0 + np.arange(1, self.shape[a]) * (2.0 / self.shape[a])
                own = rng.uniform(size=n) < 0.5
                through[own, a] = rng.choice(planes, n)[own]
        back = rng.integers(0, 4, (n, 1)) * 0.25
        pos = through - back * np.sign(dirs)
        for _ in range(3):   # (a start beyond the node: one quarter step nearer, on every moving axis alike)
            outside = np.any(np.abs(pos) > 1.375, axis=1)
            pos[outside] += 0.25 * np.sign(dirs[outside])
        assert np.all(np.abs(pos) <= 1.375)
        return pos, dirs

    def world_rays(self, compiled, node_id):
        """The launch's rays: the local rays placed by the node's compiled local_to_world (float64, as given to the
        launch and to the reference).  Family B's placement is exact: no rotation, dyadic translation."""
        pos, dirs = self.local_rays()
        M = np.asarray(compiled.local_to_world[node_id], dtype=np.float64)
        wp = pos @ M[:3, :3].T + M[:3, 3]
        wd = dirs @ M[:3, :3].T
        if self.rotate is not None:
            wd = wd / np.linalg.norm(wd, axis=1)[:, None]
        return np.ascontiguousarray(wp), np.ascontiguousarray(wd)


_FLD, _PLN = "field", "plain"
CASES = [
    Case("A-357-one-box", "A", (3, 5, 7), [(0.9, _FLD)], seed=1),
    Case("A-357-three-box-rotated", "A", (3, 5, 7), [(0.6, _FLD), (0.9, _FLD), (0.4, _FLD)], rotate=ROT,
         location=(0.3, -1.7, 2.9), seed=2),
    Case("A-119-two-tile", "A", (1, 1, 9), [(0.7, _FLD), (1.1, _FLD)], container="tile", seed=3),
    Case("A-612-field-and-plain-mesh-rotated", "A", (6, 1, 2), [(1.3, _FLD), (0.2, _PLN)], container="mesh", rotate=ROT,
         location=(-2.1, 0.4, 0.77), seed=4),
    Case("A-357-spectral-480-box-rotated", "A", (3, 5, 7), [(SPECTRUM, _FLD), (0.3, _FLD)], rotate=ROT,
         location=(0.3, -1.7, 2.9), wavelength=480.0, seed=5),
    Case("A-357-spectral-650-box-rotated", "A", (3, 5, 7), [(SPECTRUM, _FLD), (0.3, _FLD)], rotate=ROT,
         location=(0.3, -1.7, 2.9), wavelength=650.0, seed=5),
    Case("A-612-three-mesh", "A", (6, 1, 2), [(0.5, _FLD), (0.8, _FLD), (0.6, _FLD)], container="mesh", seed=6),
    Case("B-222-one-box", "B", (2, 2, 2), [(0.9, _FLD)], seed=11),
    Case("B-444-three-box-shifted", "B", (4, 4, 4), [(0.6, _FLD), (0.9, _FLD), (0.4, _FLD)], location=(2.5, -0.75, 4.0),
         seed=12),
    Case("B-812-two-tile", "B", (8, 1, 2), [(0.7, _FLD), (1.1, _FLD)], container="tile", seed=13),
    Case("B-148-field-and-plain-box", "B", (1, 4, 8), [(1.3, _FLD), (0.2, _PLN)], location=(-1.25, 0.5, 0.0), seed=14),
    Case("B-284-spectral-480-box", "B", (2, 8, 4), [(SPECTRUM, _FLD), (0.3, _FLD)], wavelength=480.0, seed=15),
]
CASE_BY_NAME = {c.name: c for c in CASES}


def references(case, compiled, node_id, pos, dirs, taus, u1s):
    """`exact_march` of every ray of a case, from the compiled scene's own tables: the node's world_to_local, the
    lattice's bounds and shape, and each component's value table as the packer is handed it."""
    f = int(compiled.node_field[node_id])
    assert f >= 0
    lower, upper = compiled.field_lower[f], compiled.field_upper[f]
    shape = tuple(int(v) for v in compiled.field_shape[f])
    assert shape == case.shape
    first, count = int(compiled.comp_start[node_id]), int(compiled.comp_count[node_id])
    assert count == len(case.coefficients)
    values = []
    for k in range(count):
        v = int(compiled.comp_values[first + k])
        at, n = int(compiled.values_start[v]), int(compiled.values_count[v])
        values.append(np.asarray(compiled.field_values[at:at + n], dtype=np.float64).reshape(shape))
    w2l = np.asarray(compiled.world_to_local[node_id], dtype=np.float64)
    alphas = case.alphas()
    return [exact_march(pos[i], dirs[i], w2l, lower, upper, shape, values, alphas, taus[i], u1s[i], case.half)
            for i in range(len(taus))]
