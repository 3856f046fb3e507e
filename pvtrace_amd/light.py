"""Light sources, rays and events.

API mirror of the reference's pvtrace/light/light.py:48-262, ray.py:16-95 and
event.py:4-16.  A `Light` is three delegates (wavelength, position, direction)
sampled in the light node's frame.  The engine recognises the built-in
delegates below — including ``functools.partial(cone, theta)`` and friends,
which the reference's vectorised emitter misses (pvtrace/engine/emit.py:62-89)
— and samples them either with seeded numpy on the host or directly on the
device; anything else falls back to one Python call per ray.
"""
from dataclasses import dataclass, replace
from enum import Enum
from typing import Optional

import numpy as np

from pvtrace_amd.lattice import Lattice, check_axis

SPEED_OF_LIGHT_CM_PER_S = 2.99792458e10


class Event(Enum):
    """What happened to a ray (codes shared with the device kernel)."""

    GENERATE = 0
    REFLECT = 1
    TRANSMIT = 2
    ABSORB = 3
    NONRADIATIVE = 4
    SCATTER = 5
    EMIT = 6
    EXIT = 7
    REACT = 8
    KILL = 9
    DETECT = 10   # absorbed at a surface by a coating's absorptivity (extension; the reference has no such event)


@dataclass(frozen=True)
class Ray:
    """Position (cm), unit direction, wavelength (nm), path length travelled
    (cm), elapsed time (s) and the name of the light/component that emitted it."""

    position: tuple
    direction: tuple
    wavelength: Optional[float]
    travelled: float = 0.0
    duration: float = 0.0
    source: Optional[str] = None

    def __repr__(self):
        fmt = lambda v: "(" + ", ".join("{:.2f}".format(c) for c in v) + ")"
        return "Ray(pos={}, dir={}, nm={:.2f})".format(
            fmt(self.position), fmt(self.direction), self.wavelength
        )

    def propagate(self, distance, refractive_index):
        pos = np.asarray(self.position, dtype=np.float64)
        step = np.asarray(self.direction, dtype=np.float64) * distance
        return replace(
            self,
            position=tuple((pos + step).tolist()),
            travelled=self.travelled + distance,
            duration=self.duration
            + distance * refractive_index / SPEED_OF_LIGHT_CM_PER_S,
        )

    def representation(self, from_node, to_node):
        return replace(
            self,
            position=from_node.point_to_node(self.position, to_node),
            direction=from_node.vector_to_node(self.direction, to_node),
        )


# -- delegate callables ---------------------------------------------------

def default_wavelength():
    return 555.0


def default_position():
    return (0.0, 0.0, 0.0)


def default_direction():
    return (0.0, 0.0, 1.0)


def rectangular_mask(X, Y):
    return (np.random.uniform(-X, X), np.random.uniform(-Y, Y), 0.0)


def circular_mask(radius):
    angle = np.random.uniform(0, 2.0 * np.pi)
    r = np.sqrt(np.random.uniform()) * radius
    return (r * np.cos(angle), r * np.sin(angle), 0.0)


def cube_mask(X, Y, Z):
    return (
        np.random.uniform(-X, X),
        np.random.uniform(-Y, Y),
        np.random.uniform(-Z, Z),
    )


class DefaultWavelength(object):
    def __call__(self):
        return default_wavelength()


class DefaultPosition(object):
    def __call__(self):
        return default_position()


class DefaultDirection(object):
    def __call__(self):
        return default_direction()


class ConstantWavelengthMask(object):
    def __init__(self, nanometers):
        self.nanometers = float(nanometers)

    def __call__(self):
        return self.nanometers


class SpectrumWavelengthMask(object):
    """Wavelengths drawn from a `Distribution` by inverse-CDF sampling."""

    def __init__(self, distribution):
        self.distribution = distribution

    def __call__(self):
        return self.distribution.sample(np.random.uniform(0, 1))


class RectangularMask(object):
    def __init__(self, x, y):
        self.x, self.y = float(x), float(y)

    def __call__(self):
        return rectangular_mask(self.x, self.y)


class CircularMask(object):
    def __init__(self, radius):
        self.radius = radius

    def __call__(self):
        return circular_mask(self.radius)


class CubeMask(object):
    def __init__(self, x, y, z):
        self.x, self.y, self.z = x, y, z

    def __call__(self):
        return cube_mask(self.x, self.y, self.z)


class PositionGrid(object):
    """A tabulated position delegate: a non-negative weight per cell of a lattice in the light's own frame (extension;
    the reference's masks are uniform).  A measured beam profile, a shaded aperture, a projected image, or the absorbed
    map of one scene as the emitter of the next.

    weights : an array of shape (nx, ny, nz), each >= 1; a 2-D array is (nx, ny, 1).  Entries are finite and >= 0, their
        sum is positive and finite.  At most 2^22 cells.
    lower, upper : 3-tuples in the light's frame.  On an axis with ONE cell both entries may be None, as in
        `CoatingPattern`: the coordinate on that axis is then exactly 0.0 and no draw is taken for it -- a flat image on
        the light's z = 0 plane is ``PositionGrid(img, (-a, -b, None), (a, b, None))``.  On every other axis both are
        finite and lower < upper.

    Anything else raises `ValueError`, each problem with its own message; the device packer refuses with the same
    words.  The sampling contract, the same on the host and on the device (include/pvtrace_hip.h, PvtSourceTables):

    1. The CDF has C_0 = 0.  C_{k+1} is the running sum of the weights in slot order (ix ny + iy) nz + iz, divided by
       the total.  The last entry is set to exactly 1.
    2. Draw u_c.  The cell is the slot k with C_k <= u_c < C_{k+1}.  It is found by the bisection the phase tables use
       (cdf[m] <= u ? a = m : b = m), so a cell of zero weight is never chosen.
    3. For each bounded axis, in the order x, y, z, draw u_a.  h_a = (upper_a - lower_a) / n_a is one division, as
       `Lattice.h` has it.  The coordinate is lower_a + ((double)i_a + u_a) * h_a: an add, a multiply and an add, with no
       fused multiply-add.
    4. In the light's draw order, these draws stand where the built-in masks' position draws stand.  That is after the
       wavelength draw of a spectrum light and before the direction draws.

    A call without arguments gives one position from numpy's global generator (`Light.emit`, the host tracer),
    `sample(n)` a bundle.
    """

    MAX_CELLS = 1 << 22
    LABEL = "position grid"

    def __init__(self, weights, lower, upper):
        label = self.LABEL
        try:
            raw = np.asarray(weights)
            if raw.dtype == object or raw.dtype.kind not in "biuf":
                raise TypeError(f"dtype {raw.dtype}")
            w = np.array(raw, dtype=np.float64)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"{label}: weights must be a numeric array ({exc})") from None
        if w.ndim == 2:
            w = w[:, :, None]
        if w.ndim != 3:
            raise ValueError(f"{label}: weights must have shape (nx, ny, nz) or (nx, ny), got {w.shape}")
        if min(w.shape) < 1:
            raise ValueError(f"{label}: shape must be >= 1 on each axis, got {w.shape}")
        if w.size > self.MAX_CELLS:
            raise ValueError(f"{label}: more than 2^22 cells, got {w.size}")
        try:
            lower, upper = tuple(lower), tuple(upper)
        except TypeError:
            raise ValueError(f"{label}: lower and upper must be 3-tuples") from None
        if len(lower) != 3 or len(upper) != 3:
            raise ValueError(f"{label}: lower and upper must be 3-tuples")
        lo, hi, bounded = [], [], []
        for a in range(3):
            if lower[a] is None or upper[a] is None:
                if not (lower[a] is None and upper[a] is None):
                    raise ValueError(f"{label}: axis {a}: lower and upper must both be None or both be numbers")
                if w.shape[a] != 1:
                    raise ValueError(f"{label}: only an axis with one cell may be unbounded, axis {a} has {w.shape[a]}")
                lo.append(0.0); hi.append(0.0); bounded.append(False)
                continue
            l, u = check_axis(lower[a], upper[a], label)
            lo.append(l); hi.append(u); bounded.append(True)
        if not np.all(np.isfinite(w)) or np.any(w < 0.0):
            raise ValueError(f"{label}: weights must be finite and >= 0")
        with np.errstate(over="ignore"):
            running = np.cumsum(w.reshape(-1))   # (C order is the slot order (ix ny + iy) nz + iz)
        total = running[-1]
        if not (np.isfinite(total) and total > 0.0):
            raise ValueError(f"{label}: the sum of the weights must be positive and finite")
        cdf = np.concatenate(([0.0], running / total))
        cdf[-1] = 1.0
        # (all axes bounded: the shared lattice itself, which `like` and the maps compare; `h` is its expression either way)
        self.lattice = Lattice(w.shape, lo, hi, label) if all(bounded) else None
        self.weights = w
        self.weights.setflags(write=False)
        self.shape = tuple(int(n) for n in w.shape)
        self.lower, self.upper, self.bounded = tuple(lo), tuple(hi), tuple(bounded)
        self.cdf = cdf
        self.cdf.setflags(write=False)

    @classmethod
    def like(cls, owner, weights=None):
        """The lattice of a `ConcentrationGrid`, `VolumeMap`, `VolumeMapResult` or `CoatingPattern`; `weights` given
        separately, or the owner's own values (`values`, `counts`, `mask`)."""
        lat = getattr(owner, "lattice", None) or getattr(getattr(owner, "spec", None), "lattice", None)
        if lat is not None:
            shape, lower, upper = lat.shape, lat.lower, lat.upper
        elif hasattr(owner, "bounded") and hasattr(owner, "mask"):
            shape = owner.shape
            lower = tuple(l if b else None for l, b in zip(owner.lower, owner.bounded))
            upper = tuple(u if b else None for u, b in zip(owner.upper, owner.bounded))
        else:
            raise ValueError(f"{cls.LABEL}: {type(owner).__name__} has no lattice")
        if weights is None:
            for name in ("values", "counts", "mask"):
                if hasattr(owner, name):
                    weights = getattr(owner, name)
                    break
            else:
                raise ValueError(f"{cls.LABEL}: {type(owner).__name__} has no values, pass the weights")
        if tuple(np.shape(weights)) != tuple(shape):
            raise ValueError(f"{cls.LABEL}: weights must have the owner's shape {tuple(shape)}, got {np.shape(weights)}")
        return cls(weights, lower, upper)

    @property
    def h(self):
        """Cell widths (upper - lower) / n per axis, `Lattice.h`'s expression; 1.0 on an axis without bounds (not read)."""
        return tuple((b - a) / float(n) if on else 1.0 for a, b, n, on in zip(self.lower, self.upper, self.shape, self.bounded))

    def cells(self, u):
        """Step 2: the slot of each draw in `u` (a scalar or an array)."""
        k = np.searchsorted(self.cdf, np.asarray(u, dtype=np.float64), side="right") - 1
        return np.minimum(k, self.cdf.size - 2)

    def positions(self, uniform, n):
        """Steps 2 and 3 for n rays, the draws taken from `uniform(n)` in the contract's order -> (n, 3)."""
        k = self.cells(uniform(n))
        index = np.unravel_index(k, self.shape)
        out = np.zeros((n, 3))
        h = self.h
        for a in range(3):
            if self.bounded[a]:
                t = index[a].astype(np.float64) + uniform(n)
                out[:, a] = self.lower[a] + t * h[a]
        return out

    def sample(self, n):
        """(n, 3) positions in the light's frame from numpy's global generator (engine/emit.py: a vectorised delegate)."""
        return self.positions(lambda m: np.random.uniform(0, 1, m), int(n))

    def __call__(self):
        return tuple(self.sample(1)[0].tolist())


class DirectionTable(object):
    """A tabulated direction delegate: a `PhaseFunctionTable` p(theta) about the light's +z -- the goniometric pattern of
    an LED, a Gaussian divergence (`ScatterLobe.gaussian(...).table`), `ScatterLobe.lambertian().table` -- that the
    device emitter samples (extension).

    table : a `PhaseFunctionTable`.  Anything else raises `ValueError`.

    The rule is the one the table's docstring states for lights (include/pvtrace_hip.h, PvtSourceTables, states the
    same): the first row is used; u1 is drawn whenever the table has several rows; u2 gives the polar cosine (steps 3
    of the table's contract), u3 the azimuth (step 4), the turn is about +z.  In the light's draw order these draws
    stand where the built-in directions' draws stand.

    A bare `PhaseFunctionTable` as a light's `direction` keeps what it always was, a user delegate sampled on the host
    through its `sample(n)`; wrapping it is what asks for the lowering.  A call without arguments gives one direction
    from numpy's global generator (`Light.emit`, the host tracer), `sample(n)` a bundle.
    """

    def __init__(self, table):
        from pvtrace_amd.material import PhaseFunctionTable

        if not isinstance(table, PhaseFunctionTable):
            raise ValueError("direction table: table must be a PhaseFunctionTable")
        self.table = table

    def sample(self, n):
        return self.table.sample(n)

    def __call__(self):
        return self.table()


class Light(object):
    """Emits rays along +z of its node unless delegates say otherwise."""

    def __init__(self, wavelength=None, position=None, direction=None, name="Light"):
        self.wavelength = default_wavelength if wavelength is None else wavelength
        self.position = default_position if position is None else position
        self.direction = default_direction if direction is None else direction
        self.name = name

    def emit(self, num_rays=None):
        if num_rays is None or num_rays == 0:
            return
        for _ in range(num_rays):
            yield Ray(
                wavelength=self.wavelength(),
                position=tuple(self.position()),
                direction=tuple(np.asarray(self.direction()).tolist()),
                source=self.name,
            )
