"""The box-shaped voxel lattice in a node's own frame that concentration fields, volume maps, path-length maps and coating
patterns stand on: the value and its validation, the cell of a point under its three range rules, and the walk from cell to
cell along a ray ("Lattices").  Pure Python and numpy."""
import math

import numpy as np


def fmin(a, b):   # C's fmin and, below, its fmax: the other operand when one is a NaN
    return a if a < b or b != b else b


def fmax(a, b):
    return a if a > b or b != b else b


def check_axis(lower, upper, label):   # one bounded axis as floats, finite and lower < upper, else ValueError led by `label`
    lo, hi = float(lower), float(upper)
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"{label}: lower and upper must be finite, got {lo} {hi}")
    if not lo < hi:
        raise ValueError(f"{label}: needs lower < upper on each axis, got {lo} {hi}")
    return lo, hi


def slot(shape, cell):   # the flattened slot (ix ny + iy) nz + iz
    return (cell[0] * shape[1] + cell[1]) * shape[2] + cell[2]


class Lattice:
    """shape (nx, ny, nz) of ints >= 1 and the box lower < upper, tuples of floats: validated, every message led by `label`."""

    def __init__(self, shape, lower, upper, label):
        try:
            self.shape = tuple(int(n) for n in shape)
        except (TypeError, ValueError):
            self.shape = ()
        if not (len(self.shape) == 3 and all(float(n) == float(m) for n, m in zip(self.shape, shape))):
            raise ValueError(f"{label}: shape must be three integers (nx, ny, nz), got {shape!r}")
        if not all(n >= 1 for n in self.shape):
            raise ValueError(f"{label}: shape must be >= 1 on each axis, got {self.shape}")
        if np.shape(lower) != (3,) or np.shape(upper) != (3,):
            raise ValueError(f"{label}: lower and upper must have three coordinates")
        self.lower, self.upper = zip(*(check_axis(lower[a], upper[a], label) for a in range(3)))

    @property
    def h(self):   # cell widths (upper - lower) / n per axis
        return tuple((b - a) / float(n) for a, b, n in zip(self.lower, self.upper, self.shape))

    def same(self, other):   # same shape, and bounds equal bit for bit
        return (self.shape, *map(float.hex, self.lower + self.upper)) == (other.shape, *map(float.hex, other.lower + other.upper))


def axis_index(p, lower, h):   # the cell rule, each one IEEE double operation; floats or arrays
    return np.floor((p - lower) / h)


def cell_clamped(p, lower, h, first, last):   # into first .. last, a NaN gives `first`: a field's 0 .. n - 1, a path map's -1 .. n
    return int(fmin(fmax(axis_index(p, lower, h), float(first)), float(last)))


def cell_inside(p, lower, h, n):   # (inside, index) for event maps and patterns: in 0 .. n - 1, which a NaN is not
    f = axis_index(p, lower, h)
    return (f >= 0.0) & (f <= n - 1.0), f


def walk(p, u, length, lower, h, shape, slabs):
    """Yields ((cx, cy, cz), s, sout) for the pieces of the ray p + s u, 0 <= s <= length, in walking order: Python floats, the
    operation order of the contracts (`ConcentrationGrid` item 3, `VolumeMap` path-length items 5-9), C's fmin / fmax.
    slabs=False: a field's interior planes 1 .. n - 1, the start clamped; slabs=True: planes 0 .. n, cells -1 .. n."""
    p, u = [float(v) for v in p], [float(v) for v in u]
    first = 0 if slabs else 1   # the first plane there is; the last is n - first, and the cells run over first - 1 .. n - first

    def ahead(a):   # the parameter of the plane ahead on axis a, inf when there is none
        i = c[a] + 1 if step[a] > 0 else c[a]
        if step[a] == 0 or i < first or i > shape[a] - first:
            return math.inf
        return (lower[a] + float(i) * h[a] - p[a]) / u[a]

    c = [cell_clamped(p[a], lower[a], h[a], first - 1, shape[a] - first) for a in range(3)]
    step = [1 if v > 0.0 else (-1 if v < 0.0 else 0) for v in u]
    t, s = [ahead(a) for a in range(3)], 0.0
    while True:
        tmin = fmin(fmin(t[0], t[1]), t[2])
        sout = fmax(fmin(tmin, length), s)
        yield (c[0], c[1], c[2]), s, sout
        if not (sout < length):
            return
        a = 0 if t[0] == tmin else (1 if t[1] == tmin else 2)   # (ties: X, then Y, then Z; the others follow at zero length)
        c[a] += step[a]
        t[a] = ahead(a)
        s = sout
