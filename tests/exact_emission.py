"""Exact references of device emission (`emit_one`) and of the built-in phase turns (`sample_phase`, and the same rule
written out at the radiative site of the trace loop), the case table, and the judges that hold the referee, the host
sampler and the kernel to them ray by ray (tests/test_emission_exact.py, tests/test_gpu_emission_exact.py).

Nothing of the product is imported here: a case is a plain `Tables` object with the fields of PvtEmitterTables
(include/pvtrace_hip.h), which the referee, the host sampler and the device all accept.  `oracle.oracle.math` supplies
the portable elementary functions (pvt_math.h), which tests/test_math.py and tests/test_gpu_parity.py pin on their own.

`stream(key, k)` -- the first k uniforms of a photon's stream: splitmix64 seeds the four words of xoshiro256+ (Vigna's
published algorithms, on Python integers), a uniform is (result >> 11) 2^-53.  `emit_key` is the emission stream of
global ray gi, ((emit_seed + gi) mod 2^64) xor 0xA5A5A5A55A5A5A5A; `trace_key` the trace stream seed + ray_offset + i
mod 2^64 (PvtTraceParams).

`kernel_emit`, `kernel_turn` -- the rule in its OWN float64 operations, one per line, in the order the contract fixes:
light gi mod n_lights; the wavelength draw first (a spectrum light only), then the position draws, then the direction
draws; the pose as ((m0 x + m1 y) + m2 z) + m3, no fused multiply-add.  float64 operations are deterministic, so the
referee and the kernel must equal them for EVERY ray: no tolerance, no ray excused.

`exact_emit`, `exact_turn` -- the same law on the exact values of the doubles: picks, comparisons, the interpolation,
positions and the Henyey-Greenstein quotient in `fractions.Fraction`, roots and circular functions (of the exact
2 pi u) in mpmath at DIGITS = 60.  Every comparison of the rule is between stored doubles (u against a CDF knot, |g|
against 2.220446049250313e-13), so the exact rule takes the same branch by construction and NO ray is ambiguous.

The bounds (U = 2^-53; `Bound` below is a running first-order analysis that keeps its second-order terms)
----------------------------------------------------------------------------------------------------------
Every value carries (x, e): x the exact value, e a bound on |computed - x|.  One operation of the rule adds the
propagated error of its operands and one rounding, U (|x| + e):
    sum            e_a + e_b                                 product   |a| e_b + |b| e_a + e_a e_b
    quotient       (|a| e_b + |b| e_a) / (|b| (|b| - e_b))   root      min(e / sqrt(x), sqrt(e))
A portable function documented to k ulp (pvt_math.h: sin, cos, sincos2pi "< 1 ulp") adds 2 k U |f| (an ulp is at most
2 U |f|) to its argument's error times a Lipschitz constant (1 for sin / cos; sincos2pi takes the draw itself, which is
exact).  IEEE sqrt adds U |f|.  What follows from that for each family:
 1. wavelength: a + (b - a)(u - c_lo) / (c_hi - c_lo) is five roundings on exact operands (two differences, the
    width, the product, the quotient) and the sum's: <= 5 U |t (b - a)| + U |r|; numpy's interp, slope first, has the
    same count.  0 where a knot value is returned (constant, histogram, the early returns, u on a knot).
 2. position: -p + 2 p u is two roundings (2 p is exact): U |2 p u| + U |r|.  The disc: ang = RN(RN(2 pi) u) is
    |RN(2 pi) - 2 pi| u + U ang away from 2 pi u, sin / cos add 2 U; rad = sqrt(u) r is 2 roundings; the product one.
 3. Henyey-Greenstein: a = 1 - g^2, d = 1 + g s, q = a / d, n = (1 + g^2) - q^2 carry about 8 U absolutely (all
    near 1), and the cosine is n / (2 g): the term U / |g| of the cancellation -- 1e-5 at |g| = 1e-11.  The exact
    cosine lies in [-1, 1], so the clamp (a projection onto an interval that holds it) never adds error.
 4. the partner sqrt((1 - c)(1 + c)): three roundings (the documented 1.3 ulp of pvt_sqrt1m2) on W = 1 - c^2, and the
    cosine's own error through the root: min(2 e_c / sqrt(W), sqrt(2 e_c)) -- the term U / sqrt(1 - c^2) near |c| = 1,
    which for Henyey-Greenstein at small |g| multiplies item 3.
 5. direction components: one product of item 4 with sin / cos of the azimuth (item 2's 2 U), one rounding.
 6. pose: three products and three (two for a direction) sums of exact matrix entries with the local components:
    sum |m_i| e_i + 3 U sum |m_i x_i| and second-order terms, through `Bound`.
A 1e-30 relative slack covers the 60-digit evaluation of the exact values.  `exact_emit` returns the draw count too.

The HOST sampler (`emit._sample_light`) takes the reference's detour through the angle: arcsin / arccos, then sin and
cos of theta and of phi = RN(RN(2 pi) u).  Its bound (`host_turn_bound`) follows ITS operations: the argument's error
through arccos / arcsin, min(e / sqrt(1 - m^2), pi sqrt(e / 2)) with m the largest |argument| within e (these
functions are Hoelder-1/2 at +-1), H_ULP ulp for every numpy function -- numpy documents its vectorised float64
functions to 4 ulp -- Lipschitz 1 through sin / cos, one product, and for Henyey-Greenstein the host's own operation
order (1 + g^2 - q^2) / (2 g).

The wrong rules (`FAULTS`) are planted in scratch copies of the referee and the host sampler on the CPU
(docs/parity_chain.md names the case each fails); here each is also a switch of `kernel_emit`, so that
tests/test_emission_exact.py can assert from the references alone that the cases see it.
"""
import bisect
import math
from fractions import Fraction as F

import mpmath
import numpy as np
from mpmath import mp, mpf

from oracle.oracle import math as portable

DIGITS = 60
MASK = (1 << 64) - 1
SALT = 0xA5A5A5A55A5A5A5A
U = 2.0 ** -53
K_EPS = 2.220446049250313e-13
H_ULP = 4.0            # numpy's documented bound for its vectorised float64 elementary functions
SLACK = 1e-30          # relative, for the 60-digit evaluation
WL_CONSTANT, WL_SPECTRUM, WL_SPECTRUM_HIST = 0, 1, 2
POS_POINT, POS_RECT, POS_CIRCLE, POS_CUBE = 0, 1, 2, 3
DIR_Z, DIR_CONE, DIR_ISOTROPIC, DIR_LAMBERTIAN, DIR_HG = 0, 1, 2, 3, 4
TWO_PI_D = 2.0 * 3.14159265358979323846     # the kernel's 2.0 * kPi, a double
FAULTS = ("bisect-lt", "searchsorted-right", "hg-draws-swapped", "cone-draws-swapped", "pose-transposed",
          "salt-dropped", "gi-mod-2^32")


# ------------------------------------------------------------------------------------------------ the stream
def _splitmix64(state):
    state = (state + 0x9E3779B97F4A7C15) & MASK
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return state, z ^ (z >> 31)


def _rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & MASK


def stream(key, k):
    """The first k uniforms of the stream `key` (any integer, taken mod 2^64), as Python floats."""
    state = key & MASK
    s = []
    for _ in range(4):
        state, word = _splitmix64(state)
        s.append(word)
    out = []
    for _ in range(k):
        result = (s[0] + s[3]) & MASK
        t = (s[1] << 17) & MASK
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = _rotl(s[3], 45)
        out.append((result >> 11) * 2.0 ** -53)       # exact: an integer below 2^53 times a power of two
    return out


def stream_array(keys, k):
    """`stream` of many keys at once, on numpy uint64 (which wraps as the algorithm asks) -> (len(keys), k) float64.  Held
    with == to `stream` in tests/test_emission_exact.py; only the hunts of 2^18 - 2^20 rays use it."""
    with np.errstate(over="ignore"):
        state = np.array([key & MASK for key in keys], dtype=np.uint64) if not isinstance(keys, np.ndarray) else keys.copy()
        s = []
        for _ in range(4):
            state = state + np.uint64(0x9E3779B97F4A7C15)
            z = state.copy()
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            s.append(z ^ (z >> np.uint64(31)))
        out = np.empty((len(state), k))
        for j in range(k):
            result = s[0] + s[3]
            t = s[1] << np.uint64(17)
            s[2] = s[2] ^ s[0]
            s[3] = s[3] ^ s[1]
            s[1] = s[1] ^ s[2]
            s[0] = s[0] ^ s[3]
            s[2] = s[2] ^ t
            s[3] = (s[3] << np.uint64(45)) | (s[3] >> np.uint64(19))
            out[:, j] = (result >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return out


def emit_keys(emit_seed, ray_offset, n):
    """`emit_key` of rays ray_offset .. ray_offset + n - 1 as a uint64 array."""
    with np.errstate(over="ignore"):
        base = np.uint64((emit_seed + ray_offset) & MASK)
        return (base + np.arange(n, dtype=np.uint64)) ^ np.uint64(SALT)


def hg_turns(g, u0, u1):
    """`kernel_turn(DIR_HG, g, .)` for arrays of draws, in numpy's float64 operations (one IEEE operation per ufunc call,
    nothing fused) and the referee's portable functions -> (directions (n, 3), the cosine before the clamp).  Held with
    == to `kernel_turn` in tests/test_emission_exact.py."""
    assert abs(g) >= K_EPS
    s = 2.0 * u0 - 1.0
    gg = g * g
    a = 1.0 - gg
    b = g * s
    d = 1.0 + b
    q = a / d
    r = 1.0 / (2.0 * g)
    n1 = 1.0 + gg
    qq = q * q
    n2 = n1 - qq
    raw = r * n2
    c = np.minimum(np.maximum(raw, -1.0), 1.0)
    w1 = 1.0 - c
    w2 = 1.0 + c
    w = w1 * w2
    sin_t = np.sqrt(w)
    cp, sp = portable("cos2pi", u1), portable("sin2pi", u1)
    return np.column_stack((sin_t * cp, sin_t * sp, c)), raw


def emit_key(emit_seed, gi, fault=None):
    if fault == "salt-dropped":
        return (emit_seed + gi) & MASK
    if fault == "gi-mod-2^32":
        return ((emit_seed + (gi & 0xFFFFFFFF)) & MASK) ^ SALT
    return ((emit_seed + gi) & MASK) ^ SALT


def trace_key(seed, ray_offset, i):
    return (seed + ray_offset + i) & MASK


# ------------------------------------------------------------------------------------------------ the tables
class Tables:
    """The fields of PvtEmitterTables over a list of lights: dict(wl=(type, value | (x, cdf)), pos=(type, (a, b, c)),
    dir=(type, param), pose=4x4)."""

    def __init__(self, lights):
        n = len(lights)
        self.n_lights = n
        self.wl_type = np.zeros(n, dtype=np.int32)
        self.wl_value = np.zeros(n)
        self.wl_spec_start = np.zeros(n, dtype=np.int32)
        self.wl_spec_n = np.zeros(n, dtype=np.int32)
        self.pos_type = np.zeros(n, dtype=np.int32)
        self.pos_param = np.zeros((n, 3))
        self.dir_type = np.zeros(n, dtype=np.int32)
        self.dir_param = np.zeros(n)
        self.light_to_world = np.zeros((n, 4, 4))
        sx, sc = [], []
        for i, light in enumerate(lights):
            kind, value = light.get("wl", (WL_CONSTANT, 555.0))
            self.wl_type[i] = kind
            if kind == WL_CONSTANT:
                self.wl_value[i] = value
            else:
                x, cdf = value
                assert len(x) == len(cdf)
                self.wl_spec_start[i], self.wl_spec_n[i] = len(sx), len(x)
                sx.extend(float(v) for v in x)
                sc.extend(float(v) for v in cdf)
            self.pos_type[i], self.pos_param[i] = light.get("pos", (POS_POINT, (0.0, 0.0, 0.0)))
            self.dir_type[i], self.dir_param[i] = light.get("dir", (DIR_Z, 0.0))
            self.light_to_world[i] = light.get("pose", np.eye(4))
        self.spec_x = np.array(sx, dtype=np.float64)
        self.spec_cdf = np.array(sc, dtype=np.float64)

    def spectrum(self, li):
        s, n = int(self.wl_spec_start[li]), int(self.wl_spec_n[li])
        return self.spec_x[s:s + n].tolist(), self.spec_cdf[s:s + n].tolist()


def rotation(angle, axis):
    """A rotation matrix as data (Rodrigues), 3 x 3 float64."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * k + (1.0 - math.cos(angle)) * (k @ k)


def pose(parent=(0.7, (0.3, -1.0, 0.6)), turn=(1.9, (1.0, 0.4, -0.2)), shift=(0.3, -1.7, 2.9), parent_shift=(5.0, 0.25, -3.0)):
    """A rotated and translated light inside a rotated and translated parent, as one 4 x 4 matrix."""
    a, b = np.eye(4), np.eye(4)
    a[:3, :3], a[:3, 3] = rotation(*parent), parent_shift
    b[:3, :3], b[:3, 3] = rotation(*turn), shift
    return a @ b


# ------------------------------------------------------------------------------------------------ portable functions
def _p(fn, x):
    return float(portable(fn, np.array([x]))[0])


def _sqrt1m2(c):
    w1 = 1.0 - c
    w2 = 1.0 + c
    w = w1 * w2
    return math.sqrt(w)


# ------------------------------------------------------------------------------------------------ the kernel's rule
def kernel_turn(kind, param, u, fault=None):
    """`sample_phase` (kind DIR_CONE / DIR_ISOTROPIC / DIR_HG) and `lambert_direction` (DIR_LAMBERTIAN) on the draws
    u[0], u[1] in stream order -> ((x, y, z) about +z, info).  info: `branch`, and for Henyey-Greenstein `raw`, the
    cosine before the clamp."""
    info = {}
    if kind == DIR_HG and abs(param) >= K_EPS:
        g = param
        g1 = u[1] if fault == "hg-draws-swapped" else u[0]
        s = 2.0 * g1 - 1.0
        gg = g * g
        a = 1.0 - gg
        b = g * s
        d = 1.0 + b
        q = a / d
        r = 1.0 / (2.0 * g)
        n1 = 1.0 + gg
        qq = q * q
        n2 = n1 - qq
        cos_t = r * n2
        info["raw"] = cos_t
        cos_t = min(max(cos_t, -1.0), 1.0)
        turn = u[0] if fault == "hg-draws-swapped" else u[1]
        sin_t = _sqrt1m2(cos_t)
        info["branch"] = "hg"
    elif kind == DIR_CONE:
        g1, g2 = (u[1], u[0]) if fault == "cone-draws-swapped" else (u[0], u[1])
        root = math.sqrt(g1)
        sp = _p("sin", param)
        sin_t = root * sp
        turn = g2
        cos_t = _sqrt1m2(sin_t)
        info["branch"] = "cone"
    elif kind == DIR_LAMBERTIAN:
        p1, p2 = u[0], u[1]
        sin_t = math.sqrt(p1)
        cos_t = _sqrt1m2(sin_t)
        turn = p2
        info["branch"] = "lambert"
    else:
        g1, g2 = u[0], u[1]
        turn = g1
        cos_t = 2.0 * g2 - 1.0
        sin_t = _sqrt1m2(cos_t)
        info["branch"] = "iso"
    sp = _p("sin2pi", turn)
    cp = _p("cos2pi", turn)
    x = sin_t * cp
    y = sin_t * sp
    return (x, y, cos_t), info


def _interp(xs, ys, x, fault=None):
    n = len(xs)
    if n == 1:
        return ys[0], "single"
    if x <= xs[0]:
        return ys[0], "below"
    if x >= xs[n - 1]:
        return ys[n - 1], "above"
    lo, hi = 0, n - 1
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if (xs[mid] < x) if fault == "bisect-lt" else (xs[mid] <= x):
            lo = mid
        else:
            hi = mid
    if xs[hi] == xs[lo]:
        return ys[lo], "flat"
    dy = ys[hi] - ys[lo]
    dx = x - xs[lo]
    w = xs[hi] - xs[lo]
    p = dy * dx
    t = p / w
    return ys[lo] + t, "inside"


def kernel_emit(tab, emit_seed, gi, fault=None):
    """`emit_one` for global ray gi -> (pos, dir, wl, draws taken, info)."""
    u = stream(emit_key(emit_seed, gi, fault), 8)
    k = 0
    li = gi % tab.n_lights
    info = {"light": li}
    wt = int(tab.wl_type[li])
    if wt in (WL_SPECTRUM, WL_SPECTRUM_HIST):
        x, cdf = tab.spectrum(li)
        uw = u[k]; k += 1
        if wt == WL_SPECTRUM_HIST:
            count = sum(1 for c in cdf if (c <= uw if fault == "searchsorted-right" else c < uw))
            wl = x[count if count < len(x) else len(x) - 1]
            info["wl_branch"] = "hist"
        else:
            wl, info["wl_branch"] = _interp(cdf, x, uw, fault)
    else:
        wl = float(tab.wl_value[li])
    lp = [0.0, 0.0, 0.0]
    pp = [float(v) for v in tab.pos_param[li]]
    pt = int(tab.pos_type[li])
    if pt in (POS_RECT, POS_CUBE):
        for a in range(2 if pt == POS_RECT else 3):
            twice = 2.0 * pp[a]
            span = twice * u[k]; k += 1
            lp[a] = -pp[a] + span
    elif pt == POS_CIRCLE:
        ang = TWO_PI_D * u[k]; k += 1
        root = math.sqrt(u[k]); k += 1
        rad = root * pp[0]
        lp[0] = rad * _p("cos", ang)
        lp[1] = rad * _p("sin", ang)
    dt = int(tab.dir_type[li])
    ld = (0.0, 0.0, 1.0)
    if dt != DIR_Z:
        ld, turn_info = kernel_turn(dt, 0.0 if dt == DIR_ISOTROPIC else float(tab.dir_param[li]), u[k:k + 2], fault)
        info.update(turn_info)
        k += 2
    m = tab.light_to_world[li]
    if fault == "pose-transposed":
        m = np.array(m)
        m[:3, :3] = m[:3, :3].T
    m = [[float(v) for v in row] for row in m]
    pos, direction = [], []
    for r in range(3):
        t0 = m[r][0] * lp[0]
        t1 = m[r][1] * lp[1]
        t2 = m[r][2] * lp[2]
        acc = t0 + t1
        acc = acc + t2
        pos.append(acc + m[r][3])
        t0 = m[r][0] * ld[0]
        t1 = m[r][1] * ld[1]
        t2 = m[r][2] * ld[2]
        acc = t0 + t1
        direction.append(acc + t2)
    return pos, direction, wl, k, info


def kernel_bundle(tab, n, emit_seed, ray_offset=0, fault=None):
    """`kernel_emit` of rays ray_offset .. ray_offset + n - 1 -> (pos (n, 3), dir (n, 3), wl (n), draws (n), infos)."""
    rows = [kernel_emit(tab, emit_seed, ray_offset + i, fault) for i in range(n)]
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]),
            np.array([r[3] for r in rows]), [r[4] for r in rows])


# ------------------------------------------------------------------------------------------------ the exact rule
class Bound:
    """(x, e): x the exact value (float magnitude, for the bound only), e a bound on |computed - x|."""

    __slots__ = ("x", "e")

    def __init__(self, x, e=0.0):
        self.x, self.e = float(x), float(e)

    def rounded(self, k=1.0):
        return Bound(self.x, self.e + k * U * (abs(self.x) + self.e))

    def __add__(self, o):
        return Bound(self.x + o.x, self.e + o.e).rounded()

    def __sub__(self, o):
        return Bound(self.x - o.x, self.e + o.e).rounded()

    def __mul__(self, o):
        return Bound(self.x * o.x, abs(self.x) * o.e + abs(o.x) * self.e + self.e * o.e).rounded()

    def __truediv__(self, o):
        assert abs(o.x) > o.e
        return Bound(self.x / o.x, (abs(self.x) * o.e + abs(o.x) * self.e) / (abs(o.x) * (abs(o.x) - o.e))).rounded()

    def sqrt(self):
        x = max(self.x, 0.0)
        e = math.sqrt(self.e) if x == 0.0 else min(self.e / math.sqrt(x), math.sqrt(self.e))
        return Bound(math.sqrt(x), e).rounded()

    def function(self, value, ulps, lipschitz=1.0):
        """A function documented to `ulps` ulp, of Lipschitz constant `lipschitz`, whose exact value is `value`."""
        return Bound(value, lipschitz * self.e + 2.0 * ulps * U * abs(float(value)))

    def clamped(self):
        return Bound(self.x, self.e)        # a projection onto an interval that holds the exact value


ONE = Bound(1.0)


def _sqrt1m2_bound(c):
    return ((ONE - c) * (ONE + c)).sqrt()


def _mp(q):
    return mpf(q.numerator) / mpf(q.denominator) if isinstance(q, F) else mpf(q)


def _hg_cosine_exact(g, u):
    g, s = F(g), 2 * F(u) - 1
    q = (1 - g * g) / (1 + g * s)
    return (1 + g * g - q * q) / (2 * g)


def _hg_cosine_bound(g, u, host=False):
    G, S = Bound(g), (Bound(2.0 * u) - ONE)
    gg = G * G
    q = (ONE - gg) / (ONE + G * S)
    n = (ONE + gg) - q * q
    if host:
        return n / Bound(2.0 * g)
    return (ONE / Bound(2.0 * g)) * n


def exact_turn(kind, param, u):
    """The law of `kernel_turn` on exact values -> (exact (x, y, z) as mpf, bounds (ex, ey, ez) as floats, branch)."""
    with mpmath.workdps(DIGITS):
        if kind == DIR_HG and abs(F(param)) >= F(K_EPS):
            c = _mp(_hg_cosine_exact(param, u[0]))
            assert -1 <= c <= 1
            s = mpmath.sqrt((1 - c) * (1 + c))
            turn = u[1]
            bc = _hg_cosine_bound(param, u[0]).clamped()
            bc.x = float(c)
            bs = _sqrt1m2_bound(bc)
            branch = "hg"
        elif kind == DIR_CONE:
            s = mpmath.sqrt(_mp(F(u[0]))) * mpmath.sin(_mp(F(param)))
            c = mpmath.sqrt((1 - s) * (1 + s))
            turn = u[1]
            bs = Bound(u[0]).sqrt() * Bound(param).function(math.sin(param), 1.0)
            bs.x = float(s)
            bc = _sqrt1m2_bound(bs)
            branch = "cone"
        elif kind == DIR_LAMBERTIAN:
            s = mpmath.sqrt(_mp(F(u[0])))
            c = mpmath.sqrt(1 - _mp(F(u[0])))
            turn = u[1]
            bs = Bound(u[0]).sqrt()
            bc = _sqrt1m2_bound(bs)
            branch = "lambert"
        else:
            c = _mp(2 * F(u[1]) - 1)
            s = mpmath.sqrt((1 - c) * (1 + c))
            turn = u[0]
            bc = Bound(2.0 * u[1]) - ONE
            bs = _sqrt1m2_bound(bc)
            branch = "iso"
        phi = 2 * mp.pi * _mp(F(turn))
        sp, cp = mpmath.sin(phi), mpmath.cos(phi)
        bx = bs * Bound(turn).function(float(cp), 1.0, lipschitz=0.0)
        by = bs * Bound(turn).function(float(sp), 1.0, lipschitz=0.0)
        exact = (s * cp, s * sp, c)
        slack = [SLACK + 1e-25 * abs(float(v)) for v in exact]
        return exact, (bx.e + slack[0], by.e + slack[1], bc.e + slack[2]), branch


def host_turn_bound(kind, param, u):
    """The bound of `exact_turn`'s value for the HOST sampler's operations (module docstring) -> (ex, ey, ez)."""
    def inverse(b):   # arccos / arcsin of an argument known to e
        m = min(abs(b.x) + b.e, 1.0)
        e = math.pi * math.sqrt(b.e / 2.0) if m >= 1.0 else min(b.e / math.sqrt((1.0 - m) * (1.0 + m)), math.pi * math.sqrt(b.e / 2.0))
        return e
    with mpmath.workdps(DIGITS):
        if kind == DIR_HG:
            arg = _hg_cosine_bound(param, u[0], host=True).clamped()
            arg.x = float(_hg_cosine_exact(param, u[0]))
            theta = math.acos(min(max(arg.x, -1.0), 1.0))
            turn = u[1]
        elif kind == DIR_CONE:
            arg = Bound(u[0]).sqrt() * Bound(param).function(math.sin(param), H_ULP)
            theta, turn = math.asin(min(arg.x, 1.0)), u[1]
        elif kind == DIR_LAMBERTIAN:
            arg = Bound(u[0]).sqrt()
            theta, turn = math.asin(arg.x), u[1]
        else:
            arg = Bound(2.0 * u[1]) - ONE
            theta, turn = math.acos(arg.x), u[0]
        bt = Bound(theta, inverse(arg) + 2.0 * H_ULP * U * abs(theta))
        phi = Bound(TWO_PI_D, abs(float(mpf(TWO_PI_D) - 2 * mp.pi))) * Bound(turn)
        st, ct = bt.function(math.sin(theta), H_ULP), bt.function(math.cos(theta), H_ULP)
        cp, sp = phi.function(math.cos(phi.x), H_ULP), phi.function(math.sin(phi.x), H_ULP)
        return ((st * cp).e + SLACK, (st * sp).e + SLACK, ct.e + SLACK)


def _exact_wavelength(x, cdf, u, hist):
    """-> (exact wavelength as Fraction, bound, branch, segment, tie)."""
    n = len(x)
    uq, cq = F(u), [F(c) for c in cdf]
    tie = uq in cq
    if hist:
        count = sum(1 for c in cq if c < uq)
        k = min(count, n - 1)
        return F(x[k]), 0.0, "hist", k, tie
    if n == 1:
        return F(x[0]), 0.0, "single", 0, tie
    if uq <= cq[0]:
        return F(x[0]), 0.0, "below", 0, tie
    if uq >= cq[-1]:
        return F(x[-1]), 0.0, "above", n - 2, tie
    lo = bisect.bisect_right(cq, uq) - 1          # the last knot at or below u (Python's own search, on Fractions)
    a, b = F(x[lo]), F(x[lo + 1])
    t = (uq - cq[lo]) / (cq[lo + 1] - cq[lo])
    value = a + t * (b - a)
    step = abs(float(t * (b - a)))
    bound = 0.0 if t == 0 else (5.0 * U * step + U * abs(float(value))) * (1.0 + 1e-9)
    return value, bound, "inside", lo, tie


def exact_position(pt, pp, u, ulps=1.0):
    """The local launch position on exact values -> (mpf triple, Bounds, draws taken); `ulps`: of sin / cos of the disc."""
    lp, bp, k = [mpf(0)] * 3, [Bound(0.0) for _ in range(3)], 0
    if pt in (POS_RECT, POS_CUBE):
        for a in range(2 if pt == POS_RECT else 3):
            lp[a] = _mp(-F(pp[a]) + 2 * F(pp[a]) * F(u[k]))
            bp[a] = Bound(-pp[a]) + Bound(2.0 * pp[a]) * Bound(u[k])
            k += 1
    elif pt == POS_CIRCLE:
        phi = 2 * mp.pi * _mp(F(u[0]))
        rad = mpmath.sqrt(_mp(F(u[1]))) * _mp(F(pp[0]))
        lp[0], lp[1] = rad * mpmath.cos(phi), rad * mpmath.sin(phi)
        ang = Bound(TWO_PI_D, abs(float(mpf(TWO_PI_D) - 2 * mp.pi))) * Bound(u[0])
        brad = Bound(u[1]).sqrt() * Bound(pp[0])
        bp[0] = brad * ang.function(float(mpmath.cos(phi)), ulps)
        bp[1] = brad * ang.function(float(mpmath.sin(phi)), ulps)
        k = 2
    for a in range(3):
        bp[a].x = float(lp[a])
    return lp, bp, k


def exact_emit(tab, emit_seed, gi):
    """The law of `kernel_emit` on exact values -> dict(pos, dir: mpf triples, wl: Fraction, e_pos, e_dir: float
    triples, e_wl, draws, light, branch, wl_branch, segment, tie)."""
    u = stream(emit_key(emit_seed, gi), 8)
    k = 0
    li = gi % tab.n_lights
    out = {"light": li, "branch": "z", "wl_branch": "constant", "segment": -1, "tie": False}
    with mpmath.workdps(DIGITS):
        wt = int(tab.wl_type[li])
        if wt == WL_CONSTANT:
            out["wl"], out["e_wl"] = F(float(tab.wl_value[li])), 0.0
        else:
            x, cdf = tab.spectrum(li)
            out["wl"], out["e_wl"], out["wl_branch"], out["segment"], out["tie"] = _exact_wavelength(
                x, cdf, u[k], wt == WL_SPECTRUM_HIST)
            k += 1
        pp = [float(v) for v in tab.pos_param[li]]
        pt = int(tab.pos_type[li])
        lp, bp, taken = exact_position(pt, pp, u[k:])
        out["pos_draws"] = u[k:k + taken]
        k += taken
        dt = int(tab.dir_type[li])
        ld, bd = [mpf(0), mpf(0), mpf(1)], [Bound(0.0), Bound(0.0), Bound(1.0)]
        if dt != DIR_Z:
            ld, ed, out["branch"] = exact_turn(dt, 0.0 if dt == DIR_ISOTROPIC else float(tab.dir_param[li]), u[k:k + 2])
            out["dir_draws"] = u[k:k + 2]
            bd = [Bound(float(v), e) for v, e in zip(ld, ed)]
            k += 2
        m = tab.light_to_world[li]
        pos, direction, e_pos, e_dir = [], [], [], []
        for r in range(3):
            row = [float(v) for v in m[r]]
            pos.append(sum(_mp(F(row[a])) * lp[a] for a in range(3)) + _mp(F(row[3])))
            direction.append(sum(_mp(F(row[a])) * ld[a] for a in range(3)))
            b = ((Bound(row[0]) * bp[0] + Bound(row[1]) * bp[1]) + Bound(row[2]) * bp[2]) + Bound(row[3])
            e_pos.append(b.e + SLACK + 1e-25 * abs(b.x))
            b = (Bound(row[0]) * bd[0] + Bound(row[1]) * bd[1]) + Bound(row[2]) * bd[2]
            e_dir.append(b.e + SLACK + 1e-25 * abs(b.x))
        out.update(pos=pos, dir=direction, e_pos=e_pos, e_dir=e_dir, draws=k, local_pos=lp, local_dir=ld, all_draws=u[:k])
    return out


_EXACT = {}


def exact_bundle(case):
    """`exact_emit` of every ray of a case, computed once."""
    if case.name not in _EXACT:
        _EXACT[case.name] = [exact_emit(case.tables, case.emit_seed, case.ray_offset + i) for i in range(case.n)]
    return _EXACT[case.name]


def worst_ratio(refs, pos, dirs, wl):
    """max |value - exact| / bound over every component of every ray (a zero bound demands equality: ratio 0 or inf)."""
    worst = 0.0
    with mpmath.workdps(DIGITS):
        for i, ref in enumerate(refs):
            pairs = [(pos[i][a], ref["pos"][a], ref["e_pos"][a]) for a in range(3)]
            pairs += [(dirs[i][a], ref["dir"][a], ref["e_dir"][a]) for a in range(3)]
            pairs.append((wl[i], _mp(ref["wl"]), ref["e_wl"]))
            for got, want, bound in pairs:
                if not math.isfinite(got):
                    return math.inf
                err = abs(float(_mp(F(float(got))) - want))
                if err > 0.0:
                    worst = max(worst, err / bound if bound > 0.0 else math.inf)
    return worst


# ------------------------------------------------------------------------------------------------ the cases
class Case:
    def __init__(self, name, lights, n=1024, emit_seed=2024, ray_offset=0, family="directions", branches=(), tied=False,
                 small_table=False, signs=True):
        self.name, self.lights, self.n, self.emit_seed, self.ray_offset = name, lights, n, emit_seed, ray_offset
        self.family, self.branches, self.tied, self.small_table, self.signs = family, branches, tied, small_table, signs
        self._tables = None

    def __repr__(self):
        return self.name

    @property
    def tables(self):
        if self._tables is None:
            lights = self.lights(self) if callable(self.lights) else self.lights
            self._tables = Tables(lights)
        return self._tables


POSE = pose()
POSE2 = pose(parent=(2.3, (-0.2, 0.5, 1.0)), turn=(0.4, (0.1, 0.9, 0.3)), shift=(-4.0, 0.5, 0.125))


def _light(**kw):
    kw.setdefault("pose", POSE)
    return kw


def _hg(g):
    return [_light(dir=(DIR_HG, g))]


def _trapezoid_cdf(x, y):
    c = np.concatenate(([0.0], np.cumsum(0.5 * (y[1:] + y[:-1]) * np.diff(x))))
    return c / c[-1]


def _first_draws(case, n_knots, lo=0.0, hi=1.0):
    """Sorted first draws of `n_knots` of the case's own rays within (lo, hi): knots that rays land on exactly."""
    draws = sorted(stream(emit_key(case.emit_seed, case.ray_offset + i), 1)[0] for i in range(0, case.n, case.n // n_knots))
    return [d for d in draws if lo < d < hi]


def _tied_linear(case):
    # every knot twice: a zero-mass segment AT a ray's own draw, where the inverse CDF jumps and the `<=` of the
    # bisection decides which side the ray gets
    knots = _first_draws(case, 128)
    cdf = [0.0] + [k for knot in knots for k in (knot, knot)] + [1.0]
    x = np.linspace(400.0, 700.0, len(cdf)) + 0.4 * np.sin(np.arange(len(cdf)))
    return [_light(wl=(WL_SPECTRUM, (np.sort(x), cdf)))]


def _tied_hist(case):
    knots = _first_draws(case, 128)
    cdf = knots + [1.0]
    return [_light(wl=(WL_SPECTRUM_HIST, (np.linspace(350.0, 900.0, len(cdf)), cdf)))]


def _big_table(case):
    rng = np.random.default_rng(11)
    x = np.sort(rng.uniform(300.0, 1100.0, 2000))
    return [_light(wl=(WL_SPECTRUM, (x, _trapezoid_cdf(x, rng.uniform(0.0, 1.0, 2000) ** 3))))]


ZERO_MASS_X = [400.0, 410.0, 450.0, 500.0, 520.0, 560.0, 600.0, 640.0, 700.0]
ZERO_MASS_CDF = [0.0, 0.0, 0.25, 0.5, 0.5, 0.5, 0.8, 1.0, 1.0]        # zero mass at the start, in the middle, at the end
SEVEN = [
    _light(wl=(WL_SPECTRUM, ([400.0, 500.0, 650.0], [0.0, 0.3, 1.0])), pos=(POS_RECT, (0.5, 1.5, 0.0)), dir=(DIR_CONE, 0.5)),
    _light(pos=(POS_CIRCLE, (2.0, 0.0, 0.0)), dir=(DIR_LAMBERTIAN, 0.0), pose=POSE2),
    _light(wl=(WL_SPECTRUM_HIST, ([410.0, 520.0, 630.0, 740.0], [0.1, 0.4, 0.8, 1.0])), pos=(POS_CUBE, (1.0, 2.0, 3.0)),
           dir=(DIR_ISOTROPIC, 0.0)),
    _light(dir=(DIR_HG, 0.7), pose=np.eye(4)),
    _light(wl=(WL_CONSTANT, 632.8), dir=(DIR_Z, 0.0), pose=POSE2),
    _light(wl=(WL_SPECTRUM, ([300.0, 800.0], [0.0, 1.0])), pos=(POS_CIRCLE, (0.25, 0.0, 0.0)), dir=(DIR_HG, -0.4)),
    _light(pos=(POS_RECT, (3.0, 0.125, 0.0)), dir=(DIR_CONE, 1.2), pose=POSE2),
]
CASES = [
    Case("D-pose-only", [_light(wl=(WL_CONSTANT, 555.0))], signs=False),
    Case("P-rect-cone-0.5", [_light(pos=(POS_RECT, (1.5, 0.25, 0.0)), dir=(DIR_CONE, 0.5))], family="positions", branches=("cone",),
         signs=False),
    Case("P-cone-half-pi", [_light(dir=(DIR_CONE, math.pi / 2))], family="positions", branches=("cone",)),
    Case("P-cone-1e-8", [_light(dir=(DIR_CONE, 1e-8))], family="positions", branches=("cone",), signs=False),
    Case("P-disc-lambert", [_light(pos=(POS_CIRCLE, (2.5, 0.0, 0.0)), dir=(DIR_LAMBERTIAN, 0.0))], family="positions",
         branches=("lambert",)),
    Case("P-cube-isotropic", [_light(pos=(POS_CUBE, (1.0, 0.5, 3.0)), dir=(DIR_ISOTROPIC, 0.0))], family="positions",
         branches=("iso",)),
    Case("H-0.9", _hg(0.9), family="hg", branches=("hg",)),
    Case("H--0.6", _hg(-0.6), family="hg", branches=("hg",)),
    Case("H-0.3", _hg(0.3), family="hg", branches=("hg",)),
    Case("H-1e-3", _hg(1e-3), family="hg", branches=("hg",)),
    Case("H-1e-11", _hg(1e-11), family="hg", branches=("hg",)),
    Case("H--1e-11", _hg(-1e-11), family="hg", branches=("hg",)),
    Case("H-3e-13", _hg(3e-13), family="hg", branches=("hg",)),
    Case("H-2e-13-isotropic", _hg(2e-13), family="hg", branches=("iso",)),
    Case("S-two-knots", [_light(wl=(WL_SPECTRUM, ([450.0, 650.0], [0.0, 1.0])))], family="spectra", branches=("inside",),
         small_table=True, signs=False),
    Case("S-2000-knots", _big_table, family="spectra", branches=("inside",), signs=False),
    Case("S-zero-mass", [_light(wl=(WL_SPECTRUM, (ZERO_MASS_X, ZERO_MASS_CDF)))], family="spectra", branches=("inside",),
         small_table=True, signs=False),
    Case("S-zero-mass-hist", [_light(wl=(WL_SPECTRUM_HIST, (ZERO_MASS_X, ZERO_MASS_CDF)))], family="spectra",
         branches=("hist",), small_table=True, signs=False),
    Case("S-short-ends", [_light(wl=(WL_SPECTRUM, ([400.0, 500.0, 600.0, 700.0], [0.08, 0.4, 0.7, 0.93])))], family="spectra",
         branches=("below", "inside", "above"), small_table=True, signs=False),
    Case("S-short-ends-hist", [_light(wl=(WL_SPECTRUM_HIST, ([400.0, 500.0, 600.0, 700.0], [0.08, 0.4, 0.7, 0.93])))],
         family="spectra", branches=("hist",), small_table=True, signs=False),
    Case("S-tied-linear", _tied_linear, family="spectra", branches=("inside",), tied=True, n=2048, signs=False),
    Case("S-tied-hist", _tied_hist, family="spectra", branches=("hist",), tied=True, n=2048, signs=False),
    Case("R-seven-lights", SEVEN, family="streams", ray_offset=1000, n=1400,
         branches=("cone", "lambert", "iso", "hg", "z")),
    Case("R-offset-2^40", SEVEN, family="streams", ray_offset=2 ** 40 + 3),
    Case("R-seed-wraps", SEVEN, family="streams", emit_seed=2 ** 64 - 100, ray_offset=0),
]
BY_NAME = {c.name: c for c in CASES}


def hg_grid():
    """200 values of g in +-[1e-12, 0.999], log-spaced in magnitude, both signs."""
    mags = np.geomspace(1e-12, 0.999, 100)
    return [float(v) for v in np.concatenate((mags, -mags))]


EDGE_DRAWS = (0.0, 2.0 ** -53, 1.0 - 2.0 ** -53)
