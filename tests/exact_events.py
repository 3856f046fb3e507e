"""Exact references of one rough-surface event and of one phase-table turn, and the ray families that hold the host
samplers and the kernel to them ray by ray (tests/test_rough_events_exact.py, tests/test_phase_turn_exact.py,
tests/test_gpu_rough_events_exact.py, tests/test_gpu_phase_turn_exact.py).

The references are written from the contract text of include/pvtrace_hip.h (PvtSurfaceTables, items 1-6;
PvtPhaseTables, items 1-4), not from the kernel or the host.  `exact_rough_event` works in mpmath at DIGITS = 60
digits; `exact_phase_turn` picks the row and inverts the CDF in `fractions.Fraction` (a linear scan for the first
segment with a larger CDF, no bisection) and forms sqrt(1 - mu^2), the azimuth and the basis in mpmath.  Every input
is the exact value of its float64.  Two things are the contract's DOUBLES: the sign of a zero N.z or d.z, which decides
s = copysign(1, z) (mpmath has no signed zero; it is read off the double), and the test "Vh.x^2 + Vh.y^2 is 0", which
the reference takes on exact values (it is exactly 0 only where every product that forms it is).

The tolerances (U = 2^-53; first order in U; every bound below is an ABSOLUTE error of a quantity of magnitude <= 1)
----------------------------------------------------------------------------------------------------------------
Constants.  pvt_sqrt and pvt_sincos2pi are within 1 ulp of the exact value (pvt_math.h: "< 1 ulp on the domains the
tracer uses", "Error < 1 ulp of the exact sin / cos of 2 pi g"; tests/test_math.py holds both to mpmath): a relative
error S U of a square root with S = 2, an absolute error T U of a sine or cosine with T = TRIG_KERNEL = 2.  The host
forms phi = fl(fl(2 pi) u) first: |d phi| <= (1 + 0.35) U 2 pi (the product's rounding and the constant's), and a libm
within 1 ulp: T = TRIG_HOST = 12.  The bound's transcendental term is the one place where host and kernel differ.
|sqrt(max(0, x + e)) - sqrt(x)| <= min(|e| / sqrt(x), sqrt(|e|)) =: rt(x, e) is used for every square root whose
argument can vanish; it is where the ill-conditioned terms come from.

Rough event (`RoughExact.bound_reflect`, `.bound_transmit`: a bound on each component of |d' - exact d'|)
 1. Basis about N (N = +-the logged normal, exact): a = -1 / (s + z) with |a| <= 1, at most four roundings per
    component: e_b = 4 U.  v_l.x, v_l.y: three products and sums of a basis vector with d, e_vl = 2 e_b + 3 U = 11 U;
    v_l.z = v.N: 3 U.
 2. Vh = normalize(alpha v_l.x, alpha v_l.y, v_l.z), len0 its length before.  The components before: 12 alpha U, 3 U.
    The length's relative error rel = (|hx| 12 alpha U + |hy| 12 alpha U + |hz| 3 U) / len0^2 + (S + 3) U -- the 3 U /
    |v.N| of a grazing ray is in here -- and e_hxy = 12 alpha U / len0 + sqrt(lensq) (rel + U), e_hz = 3 U / len0 +
    |Vh.z| (rel + U).
 3. T1 = (-Vh.y, Vh.x, 0) / sqrt(lensq): a unit vector of a vector known to e_hxy: e_T = 2 e_hxy / sqrt(lensq) +
    (S + 3) U, the U / sqrt(lensq) of near-normal incidence (0 on the fallback branch, where T1 is a constant).
    T2 = Vh x T1: e_T2xy = e_hz + e_T + U; T2.z = sqrt(lensq) is well conditioned, e_T2z = 2 e_hxy +
    1.5 sqrt(lensq) e_T + 3 U.
 4. r = sqrt(u_a) (S U r); t1 = r cos: e_t1 = (S + T + 1) U r.  s = (1 + Vh.z) / 2: e_hz / 2 + U.  A = sqrt(1 - t1^2):
    e_A = rt(1 - t1^2, 2 |t1| e_t1 + 2 U) + S U A.  t2 = (1 - s) A + s r sin: e_t2 = |r sin - A| e_s + (1 - s) e_A +
    s e_t1 + 3 U.
    tz = sqrt(max(0, X)), X = 1 - t1^2 - t2^2: e_tz = rt(X, 2 |t1| e_t1 + 2 |t2| e_t2 + 4 U) + S U tz, the U / tz term.
 5. Nh: e_Nxy = e_t1 + |t1| e_T + e_t2 + |t2| e_T2xy + sqrt(lensq) e_tz + tz e_hxy + 5 U;
    e_Nz = sqrt(lensq) e_t2 + |t2| e_T2z + |Vh.z| e_tz + tz e_hz + 3 U.  From here on the errors are 2-NORMS of
    vectors (a component's error is at most the norm's), e_Nxy that of the in-plane part of Nh.
 6. m_l = normalize(P), P = (alpha Nh.x, alpha Nh.y, max(0, Nh.z)), L = |P|.  The in-plane errors are scaled by alpha
    (which keeps a tiny alpha well conditioned at an azimuth known only to e_T), and normalising keeps only the part
    of an error across P: of the z error the share p_xy = alpha |Nh.xy| / L.
    e_ml = (alpha (e_Nxy + U) + p_xy e_Nz) / L + (S + 4) U -- the U / L term, L small where Nh.z <~ alpha.
    m = m_l.x e1 + m_l.y e2 + m_l.z N, an orthonormal frame known to 2.5 e_b (six components): e_m = e_ml + 2.5 e_b + 5 U.
 7. d.m: e_dm = e_m + 3 U.  Reflection d - 2 (d.m) m: bound_reflect = 2 e_dm + 2 |d.m| e_m + 3 U.
 8. Fresnel.  c = -d.m (e_dm); W = (1 - c)(1 + c): 2 e_dm + 3 U W; B = sqrt(W): e_B = rt(W, .) + S U B; q = n B with
    n = fl(n1 / n2): e_q = n (e_B + 2 U B).  k = sqrt(1 - q^2): e_k = rt(1 - q^2, 2 q e_q + 2 U) + S U k, the U / k term.
    a_s = (n1 c - n2 k) / (n1 c + n2 k) =: A_s / D_s with |A_s| <= D_s: e_as = 2 (n1 e_dm + n2 e_k + 3 U D_s) / D_s + U,
    a_p alike; R = (a_s^2 + a_p^2) / 2: e_R = e_as + e_ap + 3 U.
 9. Snell.  x = 1 - n^2 (1 - c^2): e_x = n^2 (2 c e_dm + 2 U) + 4 U n^2 (1 - c^2) + U; kk = sqrt(max(0, x)):
    rt(x, e_x) + S U kk (U / kk); g = kk - n c: e_g = e_kk + n e_dm + 2 U n c + U |g|; d' = n d - g m:
    bound_transmit = e_g + |g| e_m + 3 U (n + |g|).
10. Fold.  d'.N: e_tn = bound + 6 U |d'|.  The mirror d' - 2 (d'.N) N about the exact N is orthogonal: it keeps the
    norm of the error and adds its own roundings, bound + 9 U max(1, |d'|), taken for a ray that the reference folds
    and for one whose fold is ambiguous.
Each bound gets 4 U of slack for the second-order terms and is capped at 2 (a first-order bound that large says
nothing: near-normal incidence in a rotated node).

A rough ray is AMBIGUOUS when |u - R| <= e_R, when |d'.N| <= e_tn for the outcome the reference takes, when
|q - 1| <= e_q, when 0 < sqrt(lensq) < 1e-6, or when |d.N| <= 3 U (which way N faces).  Either outcome is accepted of
an ambiguous ray; its direction is held to the reference's direction for the outcome the code under test took (both
folds where the fold is the ambiguous decision).

Phase turn (`PhaseExact.bound`)
 1. t of the row pick: two differences and a quotient, |t - exact| <= 3 U t.  The CDF comparisons are between doubles
    and exact: a bisection on doubles and the linear scan on rationals choose the same segment, so |u2 - C_j| has the
    bound 0 (ambiguous only at equality, where the contract is still definite; no case has such a ray).
 2. mu = mu_j + (u2 - C_j) / (C_j+1 - C_j) (mu_j+1 - mu_j): four roundings on the increment, one on the sum:
    e_mu = 4 U |mu - mu_j| + U max(|mu|, |mu_j|).
 3. sin = sqrt(1 - mu^2): e_st = rt(1 - mu^2, 2 |mu| e_mu) + 3 U st -- the U / sqrt(1 - mu^2) term; 3 U covers
    pvt_sqrt1m2 (< 1.3 ulp) and the host's sqrt((1 - mu)(1 + mu)).
 4. d' = mu d + st (cos e1 + sin e2), e_b = 4 U per basis component:
    bound = e_mu + 2 U + 2 e_st + st (2 T + 2 e_b / U + 3) U + 4 U.
A phase ray is AMBIGUOUS when |u1 - t| <= 3 U t (t > 0); both rows are then accepted, each with its own direction.
Where the two differences and the quotient that form t are all exact, t has no error and no ray is ambiguous: the case
"on-the-pick" has wavelengths 1 + u1 between rows at 1 and 2 nm, so t = u1 EXACTLY and the contract's "u1 < t" (not
"<=") keeps the lower row; the case "on-a-knot" sets the two equal CDF entries around a zero-mass segment to one ray's
own u2, so that ray's u2 sits on the knot and the contract's "first segment with C_j+1 > u2" is the one beyond the gap.

The conditions that keep the tests from hiding a failure are `check_rough_conditions` and `check_phase_conditions`:
they are asserted from the reference's outcomes alone, so a kernel bug cannot move them.
"""
import functools
import math
from fractions import Fraction as F

import mpmath
import numpy as np
from mpmath import mp, mpf

from pvtrace_amd import (
    Box, Cylinder, Luminophore, Material, Mesh, Node, PhaseFunctionTable, Scatterer, Scene, Sphere, Surface,
)
from pvtrace_amd.material import FresnelSurfaceDelegate, RefractiveIndexTable

DIGITS = 60
precise = mpmath.workdps(DIGITS)
U = mpf(2) ** -53
S_SQRT = 2          # pvt_sqrt, numpy's sqrt: relative error <= S_SQRT U (1 ulp)
TRIG_KERNEL = 2     # pvt_sincos2pi: absolute error <= TRIG_KERNEL U (1 ulp of a value <= 1)
TRIG_HOST = 12      # numpy's cos / sin of fl(2 pi u): see the docstring
E_B = 4             # a component of the Duff basis, in U
SMALL_LENSQ = mpf(10) ** -6


def rt(x, e):
    """|sqrt(max(0, x + d)) - sqrt(max(0, x))| for |d| <= e."""
    x = max(x, mpf(0))
    if x == 0:
        return mp.sqrt(e)
    return min(e / mp.sqrt(x), mp.sqrt(e))


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def duff_basis(x, y, z, z_double):
    """(e1, e2) about the unit vector (x, y, z), the contract's expressions; s from the DOUBLE z (a signed zero)."""
    s = mpf(math.copysign(1.0, z_double))
    a = -1 / (s + z)
    b = x * y * a
    return [1 + s * x * x * a, s * b, -s * x], [b, s + y * y * a, -y]


class RoughExact:
    """What `exact_rough_event` returns.  m; R; reflected, transmitted: the folded directions (transmitted None under
    total internal reflection about m, unless q is within its bound of 1); reflected_other, transmitted_other: the
    same with the fold decided the other way; reflect: the decision u < R (False when R = 0: no draw); bound_reflect,
    bound_transmit: per component; tz, k, root_lensq: the conditioning quantities; tir: q >= 1; folded_reflect,
    folded_transmit; margins and their bounds (u_margin / e_R, fold margins / e_tn, q_margin / e_q); ambiguous and the
    decisions that are (amb_decision, amb_fold_reflect, amb_fold_transmit)."""
    __slots__ = ("m", "R", "reflected", "transmitted", "reflected_other", "transmitted_other", "reflect",
                 "bound_reflect", "bound_transmit", "tz", "k", "root_lensq", "tir", "folded_reflect", "folded_transmit",
                 "u_margin", "e_R", "q_margin", "e_q", "amb_decision", "amb_fold_reflect", "amb_fold_transmit",
                 "ambiguous", "fallback", "s_sign", "terms")

    def bound(self, reflect):
        return self.bound_reflect if reflect else self.bound_transmit


@precise
def exact_rough_event(d, N_logged, alpha, n1, n2, ua, ub, u, trig=TRIG_KERNEL):
    """Items 1-6 of the PvtSurfaceTables contract on the exact values of the doubles given: the ray's direction `d`,
    the geometric normal as logged (either orientation), the node's alpha, n1 and n2 at the photon's wavelength and
    the draws u_a, u_b, u.  `trig`: the accuracy of the sine and cosine of the code it will be compared with."""
    out = RoughExact()
    d = [mpf(float(c)) for c in d]
    Ng = [mpf(float(c)) for c in N_logged]
    alpha, n1, n2, ua, ub, u = (mpf(float(v)) for v in (alpha, n1, n2, ua, ub, u))
    # 1. frame
    along = dot(d, Ng)
    o = -1.0 if along > 0 else 1.0
    N = [mpf(o) * c for c in Ng]
    e1, e2 = duff_basis(N[0], N[1], N[2], o * float(N_logged[2]))
    out.s_sign = math.copysign(1.0, o * float(N_logged[2]))
    v = [-c for c in d]
    vl = [dot(v, e1), dot(v, e2), dot(v, N)]
    # 2. microfacet normal
    h0 = [alpha * vl[0], alpha * vl[1], vl[2]]
    len0 = mp.sqrt(dot(h0, h0))
    h = [c / len0 for c in h0]
    lensq = h[0] * h[0] + h[1] * h[1]
    root = mp.sqrt(lensq)
    out.fallback = lensq == 0
    T1 = [mpf(1), mpf(0), mpf(0)] if out.fallback else [-h[1] / root, h[0] / root, mpf(0)]
    T2 = [h[1] * T1[2] - h[2] * T1[1], h[2] * T1[0] - h[0] * T1[2], h[0] * T1[1] - h[1] * T1[0]]
    r = mp.sqrt(ua)
    phi = 2 * mp.pi * ub
    cp, sp = mp.cos(phi), mp.sin(phi)
    t1 = r * cp
    sw = (1 + h[2]) / 2
    A = mp.sqrt(1 - t1 * t1)
    t2 = (1 - sw) * A + sw * r * sp
    X = 1 - t1 * t1 - t2 * t2
    tz = mp.sqrt(max(mpf(0), X))
    Nh = [t1 * T1[c] + t2 * T2[c] + tz * h[c] for c in range(3)]
    P = [alpha * Nh[0], alpha * Nh[1], max(mpf(0), Nh[2])]
    L = mp.sqrt(dot(P, P))
    ml = [c / L for c in P]
    m = [ml[0] * e1[c] + ml[1] * e2[c] + ml[2] * N[c] for c in range(3)]
    # 3. Fresnel about m
    dm = dot(d, m)
    c = min(max(-dm, mpf(0)), mpf(1))
    n = n1 / n2
    W = (1 - c) * (1 + c)
    B = mp.sqrt(W)
    q = n * B
    out.tir = q >= 1
    k = None
    if out.tir:
        R = mpf(1)
    else:
        k = mp.sqrt(1 - q * q)
        Ds, Dp = n1 * c + n2 * k, n1 * k + n2 * c
        a_s, a_p = (n1 * c - n2 * k) / Ds, (n1 * k - n2 * c) / Dp
        R = (a_s * a_s + a_p * a_p) / 2
    # 4. decision
    out.reflect = bool(R > 0 and u < R)
    # 5, 6. directions, folded
    refl = [d[i] - 2 * dm * m[i] for i in range(3)]
    x = 1 - n * n * (1 - c * c)
    kk = mp.sqrt(max(mpf(0), x))
    g = kk - n * c
    trans = [n * d[i] - g * m[i] for i in range(3)]    # n d + (kk - n c)(-m): Snell about -m, the normal along the ray

    def mirrored(t):
        tn = dot(t, N)
        return [t[i] - 2 * tn * N[i] for i in range(3)]

    rn, tn = dot(refl, N), dot(trans, N)
    out.folded_reflect, out.folded_transmit = bool(rn < 0), bool(tn > 0)

    # ---- the bounds (docstring above) ------------------------------------------------------------------------------
    Sq, T, eb = S_SQRT * U, trig * U, E_B * U
    rel = (abs(h0[0]) * 12 * alpha * U + abs(h0[1]) * 12 * alpha * U + abs(h0[2]) * 3 * U) / (len0 * len0) + Sq + 3 * U
    e_hxy = 12 * alpha * U / len0 + root * (rel + U)
    e_hz = 3 * U / len0 + abs(h[2]) * (rel + U)
    e_T = mpf(0) if out.fallback else 2 * e_hxy / root + Sq + 3 * U
    e_T2xy = e_hz + e_T + U
    e_T2z = 2 * e_hxy + 1.5 * root * e_T + 3 * U
    e_t1 = (S_SQRT + trig + 1) * U * r
    e_s = e_hz / 2 + U
    e_A = rt(1 - t1 * t1, 2 * abs(t1) * e_t1 + 2 * U) + Sq * A
    e_t2 = abs(r * sp - A) * e_s + (1 - sw) * e_A + sw * e_t1 + 3 * U
    e_tz = rt(X, 2 * abs(t1) * e_t1 + 2 * abs(t2) * e_t2 + 4 * U) + Sq * tz
    e_Nxy = e_t1 + abs(t1) * e_T + e_t2 + abs(t2) * e_T2xy + root * e_tz + tz * e_hxy + 5 * U
    e_Nz = root * e_t2 + abs(t2) * e_T2z + abs(h[2]) * e_tz + tz * e_hz + 3 * U
    p_xy = alpha * mp.sqrt(Nh[0] * Nh[0] + Nh[1] * Nh[1]) / L
    e_ml = (alpha * (e_Nxy + U) + p_xy * e_Nz) / L + Sq + 4 * U
    e_m = e_ml + 2.5 * eb + 5 * U
    e_dm = e_m + 3 * U
    b_refl = 2 * e_dm + 2 * abs(dm) * e_m + 3 * U
    e_B = rt(W, 2 * e_dm + 3 * U * W) + Sq * B
    e_q = n * (e_B + 2 * U * B)
    if out.tir:
        e_R = mpf(0)
    else:
        e_k = rt(1 - q * q, 2 * q * e_q + 2 * U) + Sq * k
        e_as = 2 * (n1 * e_dm + n2 * e_k + 3 * U * Ds) / Ds + U
        e_ap = 2 * (n1 * e_k + n2 * e_dm + 3 * U * Dp) / Dp + U
        e_R = e_as + e_ap + 3 * U
    e_x = n * n * (2 * c * e_dm + 2 * U) + 4 * U * n * n * (1 - c * c) + U
    e_kk = rt(x, e_x) + Sq * kk
    e_g = e_kk + n * e_dm + 2 * U * n * c + U * abs(g)
    b_trans = e_g + abs(g) * e_m + 3 * U * (n + abs(g))
    norm_t = mp.sqrt(dot(trans, trans))
    e_rn = b_refl + 6 * U
    e_tn = b_trans + 6 * U * norm_t
    out.amb_fold_reflect = bool(abs(rn) <= e_rn)
    out.amb_fold_transmit = bool(abs(tn) <= e_tn)
    if out.folded_reflect or out.amb_fold_reflect:
        b_refl = b_refl + 9 * U
    if out.folded_transmit or out.amb_fold_transmit:
        b_trans = b_trans + 9 * U * max(mpf(1), norm_t)
    out.bound_reflect = min(b_refl + 4 * U, mpf(2))
    out.bound_transmit = min(b_trans + 4 * U, mpf(2))

    out.reflected = mirrored(refl) if out.folded_reflect else refl
    out.reflected_other = refl if out.folded_reflect else mirrored(refl)
    out.q_margin, out.e_q = abs(q - 1), e_q
    near_onset = bool(out.q_margin <= e_q)
    if out.tir and not near_onset:
        out.transmitted = out.transmitted_other = None
    else:
        out.transmitted = mirrored(trans) if out.folded_transmit else trans
        out.transmitted_other = trans if out.folded_transmit else mirrored(trans)
    out.m, out.R, out.tz, out.k, out.root_lensq = m, R, tz, k, root
    out.terms = {name: float(value / U) for name, value in (
        ("e_hxy", e_hxy), ("e_hz", e_hz), ("e_T", e_T), ("e_t2", e_t2), ("e_tz", e_tz), ("e_Nxy", e_Nxy), ("e_Nz", e_Nz),
        ("e_ml", e_ml), ("e_m", e_m), ("e_q", e_q), ("e_R", e_R), ("e_g", e_g))}   # (in units of U, for a failure's report)
    out.u_margin, out.e_R = (abs(u - R) if R > 0 else None), e_R
    out.amb_decision = bool((R > 0 and not out.tir and out.u_margin <= e_R) or near_onset)
    unsure_frame = bool((0 < root < SMALL_LENSQ) or abs(along) <= 3 * U)
    fold_now = out.amb_fold_reflect if out.reflect else out.amb_fold_transmit
    out.ambiguous = bool(out.amb_decision or unsure_frame or fold_now)
    return out


class PhaseExact:
    """What `exact_phase_turn` returns.  row: the row picked; rows: {row: (segment, mu, direction, bound)} of every row
    the pick may take (two when |u1 - t| is within its bound, else one); t, t_margin; segment, mu, direction, bound: those
    of `row`; ambiguous; neighbours: the (lower, upper) rows the wavelength lies between, None at or beyond an end or on
    a row; s_sign: the basis's s."""
    __slots__ = ("row", "rows", "t", "t_margin", "segment", "mu", "direction", "bound", "ambiguous", "neighbours",
                 "s_sign")


def is_double(q):
    """Whether the rational q is a float64."""
    return F(float(q)) == q


def pick_row(wavelengths, wl, u1):
    """Item 2 on exact rationals -> (row, t, (k, k + 1) or None, the bound on |t - exact t| of a t formed in doubles).
    The bound is 3 U t (two differences and a quotient), and 0 where all three are exact: operations without a
    rounding have no error, whoever performs them."""
    xs = [F(float(w)) for w in wavelengths]
    lam = min(max(F(float(wl)), xs[0]), xs[-1])
    if lam >= xs[-1]:
        return len(xs) - 1, F(0), None, F(0)
    k = max(i for i in range(len(xs) - 1) if xs[i] <= lam)
    num, den = lam - xs[k], xs[k + 1] - xs[k]
    t = num / den
    exact = is_double(num) and is_double(den) and is_double(t)
    return (k + 1 if F(float(u1)) < t else k), t, ((k, k + 1) if t > 0 else None), (F(0) if exact else 3 * F(1, 2 ** 53) * t)


_ROW_FRACTIONS = {}


def _row_fractions(cdf_row):
    """The exact values of a CDF row's doubles, converted once per row (keyed by the row's bytes)."""
    key = np.ascontiguousarray(cdf_row, dtype=np.float64).tobytes()
    if key not in _ROW_FRACTIONS:
        _ROW_FRACTIONS[key] = [F(float(c)) for c in cdf_row]
    return _ROW_FRACTIONS[key]


def invert_cdf(mu_axis, cdf_row, u2):
    """Item 3 on exact rationals -> (segment j, mu): the first segment with C_j+1 > u2, by a linear scan."""
    u2 = F(float(u2))
    cs = _row_fractions(cdf_row)
    j = next(i for i in range(len(cs) - 1) if cs[i + 1] > u2)
    a, b = F(float(mu_axis[j])), F(float(mu_axis[j + 1]))
    mu = a + (u2 - cs[j]) / (cs[j + 1] - cs[j]) * (b - a)
    return j, min(max(mu, F(-1)), F(1))


@precise
def exact_phase_turn(table, wl, d, u1, u2, u3, trig=TRIG_KERNEL):
    """Items 2-4 of the PvtPhaseTables contract.  `table`: anything with the compiled table's doubles as `.wavelength`
    (None or one per row), `.mu` and `.cdf` (rows x points); wl: the photon's wavelength; d: its incoming direction;
    u1 (read only when the table has several rows), u2, u3: the draws."""
    out = PhaseExact()
    nw = len(table.cdf)
    out.t, out.t_margin, out.neighbours, candidates = F(0), None, None, [0]
    if nw > 1:
        row, t, out.neighbours, t_bound = pick_row(table.wavelength, wl, u1)
        out.t, out.t_margin = t, abs(F(float(u1)) - t)
        candidates = [row]
        if t > 0 and t_bound > 0 and out.t_margin <= t_bound:
            candidates = [row, out.neighbours[0] + out.neighbours[1] - row]
    dd = [mpf(float(c)) for c in d]
    e1, e2 = duff_basis(dd[0], dd[1], dd[2], float(d[2]))
    out.s_sign = math.copysign(1.0, float(d[2]))
    phi = 2 * mp.pi * mpf(float(u3))
    cp, sp = mp.cos(phi), mp.sin(phi)
    out.rows = {}
    for row in candidates:
        j, mu_q = invert_cdf(table.mu, table.cdf[row], u2)
        mu = mpf(mu_q.numerator) / mpf(mu_q.denominator)
        mu_j = mpf(float(table.mu[j]))
        st = mp.sqrt(max(mpf(0), 1 - mu * mu))
        direction = [mu * dd[c] + st * (cp * e1[c] + sp * e2[c]) for c in range(3)]
        e_mu = 4 * U * abs(mu - mu_j) + U * max(abs(mu), abs(mu_j))
        e_st = rt(1 - mu * mu, 2 * abs(mu) * e_mu) + 3 * U * st
        bound = e_mu + 2 * U + 2 * e_st + st * (2 * trig + 2 * E_B + 3) * U + 4 * U
        out.rows[row] = (j, mu_q, direction, bound)
    out.row = candidates[0]
    out.segment, out.mu, out.direction, out.bound = out.rows[out.row]
    out.ambiguous = len(candidates) > 1
    return out


def check_cdf_rows(table, who):
    """Item 1 of the PvtPhaseTables contract on a compiled table, in exact rationals: each row is the trapezoid integral
    of p in mu with a leading 0, divided by its last entry.  The host forms each term 0.5 (p_j + p_j+1)(mu_j+1 - mu_j)
    with three roundings (the half is exact), sums j + 1 of them in order (numpy's cumsum along a row), and divides by
    the total, itself a sum of n - 1 terms: entry j is within (3 + j + 3 + (n - 1) + 1) U = (n + j + 6) U of the exact
    quotient, relatively (all terms are >= 0).  Returns the worst |C_j - exact| / (U exact)."""
    mu = [F(float(m)) for m in table.mu]
    assert mu[0] == -1 and mu[-1] == 1 and all(a < b for a, b in zip(mu, mu[1:]))
    n = len(mu)
    values = np.atleast_2d(table.values)
    worst = 0.0
    for row in range(len(table.cdf)):
        p = [F(float(v)) for v in values[row][::-1]]
        exact, running = [F(0)], F(0)
        for j in range(n - 1):
            running += (p[j] + p[j + 1]) / 2 * (mu[j + 1] - mu[j])
            exact.append(running)
        got = [F(float(c)) for c in table.cdf[row]]
        assert got[0] == 0 and got[-1] == 1 and all(a <= b for a, b in zip(got, got[1:]))
        for j in range(1, n):
            want = exact[j] / exact[-1]
            err = abs(got[j] - want)
            assert err <= (n + j + 6) * F(1, 2 ** 53) * want, (who, row, j, float(err / want) * 2 ** 53)
            if want:
                worst = max(worst, float(err / want) * 2 ** 53)
    return worst


# ---- judging a case -------------------------------------------------------------------------------------------------------
@precise
def component_error(got, want):
    """max over the components of |got - want|, got doubles, want mpf."""
    return max(abs(mpf(float(got[c])) - want[c]) for c in range(3))


@precise
def rough_ratio(r, reflect, direction):
    """|direction - exact| / bound of one ray for the kind the code under test took (the nearer fold where the fold is
    the ambiguous decision); infinity where the reference has no direction of that kind."""
    want = r.reflected if reflect else r.transmitted
    if want is None:
        return math.inf
    err = component_error(direction, want)
    if (r.amb_fold_reflect if reflect else r.amb_fold_transmit):
        err = min(err, component_error(direction, r.reflected_other if reflect else r.transmitted_other))
    return float(err / r.bound(reflect))


@precise
def judge_draw_order(case, refs_skipped, refs_drawn, got, who):
    """The SECOND rough event of rays whose first was at an index-matched rough interface.  There the contract's R is 0
    and u is not drawn; the code under test decides on ITS R, which is 0 or a rounding residue (see the case
    G-nested-matched-0.3), so the second event's u_a, u_b, u sit at stream positions 2, 3, 4 (`refs_skipped`) or 3, 4,
    5 (`refs_drawn`).  Every ray must agree, in kind and direction, with exactly one of the two, and both must occur:
    code that always draws, never draws, or draws anything else between the events fails.  Returns the two counts."""
    skipped = drawn = 0
    for i, (a, b, (reflect, direction)) in enumerate(zip(refs_skipped, refs_drawn, got)):
        fits = [(r.amb_decision or bool(reflect) == r.reflect) and rough_ratio(r, reflect, direction) <= 1.0 for r in (a, b)]
        assert fits[0] != fits[1], (who, case, i, "the second event fits", fits, bool(reflect), [float(c) for c in direction])
        skipped += fits[0]
        drawn += fits[1]
    print(f"{who} {case}: second event after n1 = n2: u skipped by {skipped} rays, drawn by {drawn}")
    assert skipped and drawn, (who, case, "u after a matched interface: skipped, drawn", skipped, drawn)
    return skipped, drawn


@precise
def judge_rough(case, refs, got, who):
    """The checks of one rough case, shared by the host and the GPU test.  `got` per ray: (reflect, direction).
    Returns (worst |direction - exact| / bound over the unambiguous rays, the same over the ambiguous ones)."""
    worst, worst_amb = 0.0, 0.0
    for i, (r, (reflect, direction)) in enumerate(zip(refs, got)):
        if not r.amb_decision:
            assert bool(reflect) == r.reflect, (who, case, i, "kind", reflect, float(r.R), r.u_margin and float(r.u_margin))
        want = r.reflected if reflect else r.transmitted
        assert want is not None, (who, case, i, "transmitted under total internal reflection", float(r.q_margin))
        ratio = rough_ratio(r, reflect, direction)
        assert ratio <= 1.0, (who, case, i, "REFLECT" if reflect else "TRANSMIT", [float(c) for c in direction],
                              [float(c) for c in want], ratio, float(r.bound(reflect)), r.ambiguous, r.terms)
        if r.ambiguous:
            worst_amb = max(worst_amb, ratio)
        else:
            worst = max(worst, ratio)
    print(f"{who} {case}: worst |direction - exact| / bound {worst:.3f}; {sum(r.ambiguous for r in refs)} ambiguous of "
          f"{len(refs)}, worst among them {worst_amb:.3f}")
    return worst, worst_amb


@precise
def check_rough_conditions(case, refs):
    """The fixed rules of a rough case, from the reference's outcomes alone."""
    n = len(refs)
    assert 1000 <= n <= 1500, (case, n)
    ambiguous = sum(r.ambiguous for r in refs)
    if case.family == "generic":
        tight = sum(r.bound(r.reflect) < mpf(10) ** -12 for r in refs)
        assert tight * 100 >= 99 * n, (case, "direction bounds below 1e-12", tight, n)
        assert ambiguous * 100 <= n, (case, "ambiguous", ambiguous, n)
        # (n1 = n2: the contract's R is 0 and the reference never reflects; every other generic case sees both kinds)
        if not case.matched:
            assert any(r.reflect for r in refs) and any(not r.reflect for r in refs), (case, "kinds")
    else:
        assert ambiguous * 10 <= n, (case, "ambiguous", ambiguous, n)
    if case.dense_inside:
        assert any(r.tir for r in refs), (case, "no total internal reflection about m")
        assert any(r.folded_reflect if r.reflect else r.folded_transmit for r in refs), (case, "no fold")
    if case.family == "generic" and case.geometry in ("box", "mesh"):
        assert {r.s_sign for r in refs} == {1.0, -1.0}, (case, "both halves of the basis")
    if case.expects_fallback:
        assert sum(r.fallback for r in refs) * 2 >= n, (case, "the T1 fallback")
    elif case.family == "generic":
        assert not any(r.fallback for r in refs), case


@precise
def judge_phase(case, refs, got, who):
    """The checks of one phase case: `got` per ray a direction, or None for a ray that is not judged (not absorbed).
    Returns (worst ratio over the unambiguous rays, worst over the ambiguous ones)."""
    worst, worst_amb = 0.0, 0.0
    for i, (r, direction) in enumerate(zip(refs, got)):
        if direction is None:
            continue
        ratio = min(float(component_error(direction, want) / bound) for (_, _, want, bound) in r.rows.values())
        assert ratio <= 1.0, (who, case, i, [float(c) for c in direction], [float(c) for c in r.direction],
                              float(r.bound), r.row, r.segment, r.ambiguous)
        if r.ambiguous:
            worst_amb = max(worst_amb, ratio)
        else:
            worst = max(worst, ratio)
    print(f"{who} {case}: worst |direction - exact| / bound {worst:.3f}; {sum(r.ambiguous for r in refs)} ambiguous of "
          f"{len(refs)}, worst among them {worst_amb:.3f}; {sum(g is not None for g in got)} judged")
    return worst, worst_amb


SEEN_MASS = F(1, 2 ** 53)   # a thinner segment holds no draw of the 2^-53 lattice but a knot: it cannot be "seen"


@precise
def check_phase_conditions(case, refs, judged=None):
    """The fixed rules of a phase case, from the reference's outcomes alone (`judged`: the rays that count)."""
    table = case.table
    n = len(refs)
    assert 1000 <= n <= 1500, (case, n)
    use = [r for i, r in enumerate(refs) if judged is None or judged[i]]
    assert len(use) * 10 >= 4 * n, (case, "rays absorbed", len(use), n)
    assert sum(r.ambiguous for r in refs) * 100 <= n, (case, "ambiguous")
    tight = sum(r.bound < mpf(10) ** -12 for r in use)
    assert tight * 100 >= 99 * len(use), (case, "direction bounds below 1e-12", tight, len(use))
    assert {r.s_sign for r in use} == {1.0, -1.0}, (case, "both halves of the basis")
    if len(table.mu) <= 16:
        for row in {r.row for r in use}:
            cs = [F(float(c)) for c in table.cdf[row]]
            massive = {j for j in range(len(cs) - 1) if cs[j + 1] - cs[j] > SEEN_MASS}
            seen = {r.segment for r in use if r.row == row}
            assert seen <= {j for j in range(len(cs) - 1) if cs[j + 1] > cs[j]}, (case, "a zero-mass segment", row)
            assert massive <= seen, (case, "segments never seen", row, sorted(massive - seen))
    if case.special == "on-the-pick":
        assert sum(r.t_margin == 0 and not r.ambiguous and r.row == 0 for r in use) * 4 >= len(use), (case, "u1 = t")
    if case.special == "on-a-knot":
        r = refs[case.on_knot]
        assert (judged is None or judged[case.on_knot]) and r.segment == 4 and r.mu == F(float(table.mu[4])), (case, "knot")
    if len(table.cdf) > 1:
        pairs = {r.neighbours for r in use if r.neighbours is not None}
        assert pairs, (case, "no wavelength between two rows")
        for lo, hi in pairs:
            took = {r.row for r in use if r.neighbours == (lo, hi)}
            assert took == {lo, hi}, (case, "rows picked between", lo, hi, took)


# ---- the rough cases -------------------------------------------------------------------------------------------------------
ROT = (0.7, (0.3, -1.0, 0.6))
INDEX_TABLE = RefractiveIndexTable([400.0, 500.0, 650.0, 800.0], [1.62, 1.51, 1.47, 1.40])
N_GLASS = 1.5
FOLD_RAYS = 4
SEED = 5200    # ray i of a case draws from the stream SEED + i


class RoughCase:
    """One rough node, its placement, and the rays of its family.  geometry: "box" (2 x 2 x 2), "sphere" (radius 1),
    "cylinder" (length 2, radius 0.7), "mesh" (the box as 12 triangles), "tile" (the middle tile of a 6 x 6 array,
    the kernel's node grid), "nested" (a 4 x 4 x 4 box that holds a rough 2 x 2 x 2 box of n = 1.5; every ray starts
    outside and crosses both: tests/test_gpu_rough_events_exact.py reads its second event).  index: the node's index in an n = 1 world (a number or INDEX_TABLE); rays started inside
    meet (n1, n2) = (index, 1), rays started outside (1, index)."""

    def __init__(self, name, family, geometry, alpha, index=N_GLASS, rotate=None, location=None, rays="generic",
                 wavelengths=(555.0,), seed=1, n=1000):
        self.name, self.family, self.geometry, self.alpha, self.index = name, family, geometry, float(alpha), index
        self.rotate, self.location, self.rays, self.wavelengths, self.seed, self.n = rotate, location, rays, wavelengths, seed, n
        self.matched = index == 1.0
        # (half the rays of every family but "nested" start inside: n1 = index > n2 = 1 unless the indices match)
        self.dense_inside = not self.matched
        self.expects_fallback = rays == "normal"

    def __repr__(self):
        return self.name

    def scene(self, alpha=None):
        """(scene, the rough node); `alpha` overrides the case's (0: the smooth anchor)."""
        alpha = self.alpha if alpha is None else alpha
        world = Node(name="world", geometry=Box((200.0, 200.0, 200.0), material=Material(refractive_index=1.0)))
        material = Material(refractive_index=self.index, surface=Surface(FresnelSurfaceDelegate(roughness=alpha)))
        if self.geometry == "sphere":
            geometry = Sphere(1.0, material=material)
        elif self.geometry == "cylinder":
            geometry = Cylinder(2.0, 0.7, material=material)
        elif self.geometry == "mesh":
            geometry = Mesh.box((2.0, 2.0, 2.0), material=material)
        elif self.geometry == "nested":
            geometry = Box((4.0, 4.0, 4.0), material=material)
        else:
            geometry = Box((2.0, 2.0, 2.0), material=material)
        if self.geometry == "tile":
            block = None
            for i in range(36):
                row, col = divmod(i, 6)
                mine = i == 21
                # (the tracer takes the NEXT node a ray crosses beyond a surface as the adjacent one -- the reference's rule
                # -- so the other tiles have the world's index: n2 = 1 for every ray that leaves the rough tile)
                g = geometry if mine else Box((2.0, 2.0, 2.0), material=Material(refractive_index=1.0))
                tile = Node(name=f"tile-{row}-{col}", parent=world, geometry=g)
                tile.location = ((col - 2.5) * 8.0, (row - 2.5) * 8.0, 0.0)
                block = tile if mine else block
        else:
            block = Node(name="block", parent=world, geometry=geometry)
            if self.geometry == "nested":
                glass = Material(refractive_index=N_GLASS, surface=Surface(FresnelSurfaceDelegate(roughness=alpha)))
                Node(name="inner", parent=block, geometry=Box((2.0, 2.0, 2.0), material=glass))
            if self.rotate is not None:
                block.rotate(*self.rotate)
            if self.location is not None:
                block.translate(self.location)
        return Scene(world), block

    def contains(self, p):
        """Whether the node's shape holds the local points p (n, 3)."""
        if self.geometry == "sphere":
            return np.sum(p * p, axis=1) < 1.0
        if self.geometry == "cylinder":
            return (np.abs(p[:, 2]) < 1.0) & (p[:, 0] ** 2 + p[:, 1] ** 2 < 0.49)
        return np.all(np.abs(p) < 1.0, axis=1)

    def local_rays(self):
        """(positions, directions, inside) in the node's frame.  Every ray's first crossing is the node's own surface:
        it starts inside the shape, or outside it on a line through a point inside it.  A case whose alpha is at most
        1e-3 gives FOLD_RAYS of its rays to grazing incidence from inside at 0.1 alpha to alpha from the face, chosen
        among its last 400 as the first that the reference folds: no other ray of such a case can be folded."""
        rng = np.random.default_rng(self.seed)
        n = self.n
        if self.rays == "generic":
            target = np.zeros((0, 3))
            while len(target) < n:   # points inside the shape, shrunk by a tenth
                p = rng.uniform(-1.0, 1.0, (4 * n, 3))
                target = np.vstack([target, 0.9 * p[self.contains(p)]])
            target = target[:n]
            v = rng.normal(size=(n, 3))
            v /= np.linalg.norm(v, axis=1)[:, None]
            inside = np.arange(n) % 2 == 0
            pos = np.where(inside[:, None], target, target - 3.5 * v)
            if self.geometry == "nested":   # all from outside the outer box, aimed at a point of the inner one
                inside[:] = False
                pos = target - 6.0 * v
        else:
            pos, v, inside, _ = self.face_rays(rng, n, self.rays)
        if self.alpha <= 1e-3:
            assert self.geometry in ("box", "mesh")
            from oracle import oracle as O
            found = 0
            for i in range(n - 1, max(n - 401, -1), -1):   # (a fold needs draws that tilt m along the ray: about 1 ray in 25)
                ua, ub, u = O.uniforms(SEED + i, 3)
                p1, v1, _, face = self.face_rays(rng, 6, "fold")
                j = i % 6
                if exact_rough_event(v1[j], face[j], self.alpha, self.index, 1.0, ua, ub, u).folded_reflect:
                    pos[i], v[i], inside[i] = p1[j], v1[j], True
                    found += 1
                    if found == FOLD_RAYS:
                        break
        return pos, v, inside

    def face_rays(self, rng, n, kind):
        """n rays aimed at points of the six faces of the 2 x 2 x 2 box, in turn, alternately from inside and outside."""
        axes = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
        face = axes[np.arange(n) % 6]                                # the face's outward normal
        inside = (np.arange(n) // 6) % 2 == 0
        if kind in ("critical", "fold"):
            inside[:] = True
        a = np.argmax(np.abs(face), axis=1)
        b, c = (a + 1) % 3, (a + 2) % 3
        rows = np.arange(n)
        hitp = rng.uniform(-0.8, 0.8, (n, 3))
        hitp[rows, a] = face[rows, a]                                # a point of the face
        side = np.where(inside, 1.0, -1.0)[:, None]                  # the ray runs along +face from inside, -face from outside
        tang = np.zeros((n, 3))
        az = rng.uniform(0.0, 2.0 * np.pi, n)
        tang[rows, b], tang[rows, c] = np.cos(az), np.sin(az)
        back = np.full((n, 1), 0.1)
        if kind == "normal":        # exactly along the axis; the other components zeros of either sign
            v = side * face
            zero = np.where(rng.uniform(size=(n, 3)) < 0.5, 0.0, -0.0)
            v = np.where(v != 0.0, v, zero)
        elif kind in ("grazing", "fold"):     # d.N from -1e-3 to -1e-9; "fold": from -alpha to -0.1 alpha
            gcos = 10.0 ** rng.uniform(-9.0, -3.0, n) if kind == "grazing" else self.alpha * 10.0 ** rng.uniform(-1.0, 0.0, n)
            v = side * gcos[:, None] * face + np.sqrt(1.0 - gcos * gcos)[:, None] * tang
            back = np.where(inside, 0.1, 50.0)[:, None]              # (from outside: a start well clear of the face's plane)
        elif kind == "critical":    # from inside, within 1e-6 rad of the critical angle of the smooth face
            theta = math.asin(1.0 / self.index) + rng.uniform(-1e-6, 1e-6, n)
            v = np.cos(theta)[:, None] * face + np.sin(theta)[:, None] * tang
        else:                       # "in-plane": one tangential component an exact zero of either sign
            theta = rng.uniform(0.05, 1.5, n)
            which = rng.uniform(size=n) < 0.5
            tang[:] = 0.0
            tang[rows, np.where(which, b, c)] = np.where(rng.uniform(size=n) < 0.5, 1.0, -1.0)
            tang[rows, np.where(which, c, b)] = np.where(rng.uniform(size=n) < 0.5, 0.0, -0.0)
            v = side * np.cos(theta)[:, None] * face + np.sin(theta)[:, None] * tang
        return hitp - back * v, v, inside, face

    def world_rays(self, compiled, node_id):
        """(positions, directions, wavelengths, inside): the local rays placed by the node's compiled local_to_world;
        the wavelengths cycle through the case's."""
        pos, dirs, inside = self.local_rays()
        M = np.asarray(compiled.local_to_world[node_id], dtype=np.float64)
        wp = pos @ M[:3, :3].T + M[:3, 3]
        wd = dirs @ M[:3, :3].T
        if self.rotate is not None:
            wd = wd / np.linalg.norm(wd, axis=1)[:, None]
        wl = np.asarray(self.wavelengths, dtype=np.float64)[np.arange(self.n) % len(self.wavelengths)]
        return np.ascontiguousarray(wp), np.ascontiguousarray(wd), wl, inside

    def indices(self, wl, inside):
        """(n1, n2) of every ray, as doubles: a table through the referee's lookup, which is the kernel's to the bit."""
        from oracle import oracle as O
        if isinstance(self.index, RefractiveIndexTable):
            n = np.array([O.index_at(self.index.wavelength, self.index.values, w) for w in wl])
        else:
            n = np.full(len(wl), float(self.index))
        return np.where(inside, n, 1.0), np.where(inside, 1.0, n)


ROUGH_CASES = [
    RoughCase("G-box-0.3", "generic", "box", 0.3, seed=1),
    RoughCase("G-box-1e-4", "generic", "box", 1e-4, seed=2),
    RoughCase("G-box-1.0", "generic", "box", 1.0, seed=3),
    RoughCase("G-box-rotated-0.05", "generic", "box", 0.05, rotate=ROT, location=(0.3, -1.7, 2.9), seed=4),
    RoughCase("G-sphere-0.3", "generic", "sphere", 0.3, location=(1.1, 0.2, -0.4), seed=5),
    RoughCase("G-cylinder-rotated-0.05", "generic", "cylinder", 0.05, rotate=ROT, seed=6),
    RoughCase("G-cylinder-1.0", "generic", "cylinder", 1.0, seed=7),
    RoughCase("G-mesh-0.3", "generic", "mesh", 0.3, seed=8),
    RoughCase("G-mesh-rotated-1e-4", "generic", "mesh", 1e-4, rotate=ROT, location=(-2.1, 0.4, 0.77), seed=9),
    RoughCase("G-tile-0.3", "generic", "tile", 0.3, seed=10),
    RoughCase("G-box-matched-0.3", "generic", "box", 0.3, index=1.0, seed=11),
    RoughCase("G-box-rotated-index-table-0.3", "generic", "box", 0.3, index=INDEX_TABLE, rotate=ROT,
              location=(0.3, -1.7, 2.9), wavelengths=(450.0, 700.0), seed=12),
    RoughCase("G-nested-matched-0.3", "generic", "nested", 0.3, index=1.0, seed=13),
    RoughCase("E-normal-0.3", "edge", "box", 0.3, rays="normal", seed=21, n=1002),
    RoughCase("E-normal-1.0", "edge", "box", 1.0, rays="normal", seed=22, n=1002),
    RoughCase("E-grazing-0.3", "edge", "box", 0.3, rays="grazing", seed=23, n=1002),
    RoughCase("E-critical-1e-4", "edge", "box", 1e-4, rays="critical", seed=24, n=1002),
    RoughCase("E-critical-0.05", "edge", "box", 0.05, rays="critical", seed=25, n=1002),
    RoughCase("E-in-plane-0.3", "edge", "box", 0.3, rays="in-plane", seed=26, n=1002),
    RoughCase("E-in-plane-mesh-1.0", "edge", "mesh", 1.0, rays="in-plane", seed=27, n=1002),
]
ROUGH_BY_NAME = {c.name: c for c in ROUGH_CASES}
# The edge cases and the decisions they sit on.  "normal": Vh.x = Vh.y = 0 exactly, the fallback T1 = (1, 0, 0), on all
# six faces from both sides, the tangential zeros of either sign.  "grazing": v.N down to 1e-9, the 3 U / |v.N| of the
# bound's item 2.  "critical": the smooth face's critical angle from inside; about m the event sits NEAR the onset of
# total internal reflection, not on it (m is drawn: q - 1 is of the order of alpha), so about half of its rays are
# totally reflected about m and the others have a small k -- the U / k and U / kk terms; a ray whose q is within its
# bound of 1 is ambiguous and held for both outcomes.  "in-plane": hx = 0 or hy = 0 exactly.
#
# n1 = n2 and the draw u.  The contract's R is exactly 0 at n1 = n2, so by items 4 and 7 u is not drawn.  The host and the
# kernel decide "R > 0" on the R they COMPUTE: a_s = (n c - n k) / (n c + n k) with k = sqrt(1 - (1 - c)(1 + c)) is 0
# only where that k rounds to c itself, and a residue of rounding otherwise (up to 2e-12 was seen).  So the kernel draws
# u after some index-matched events (189 of the 1000 of G-nested-matched-0.3 on an MI355X), the reference after none.  The first event cannot show it: its kind is TRANSMIT unless u < 2e-12 and its direction
# does not depend on u; G-box-matched-0.3 holds those two and nothing about u.  What the draw changes is the position of
# every LATER draw, so G-nested-matched-0.3 puts a second rough interface (1 -> 1.5) behind the matched one and
# `judge_draw_order` holds the second event to the reference at either position, ray by ray, and needs both to occur.


_ROUGH_CACHE = {}


def rough_refs(case, dirs, normals, n1, n2, draws, trig):
    """`exact_rough_event` of every ray of a case, computed once per (case, normals, trig)."""
    key = (case.name, trig, np.asarray(normals, dtype=np.float64).tobytes(), np.asarray(dirs).tobytes(),
           np.asarray(draws).tobytes(), np.asarray(n2).tobytes())
    if key not in _ROUGH_CACHE:
        _ROUGH_CACHE[key] = [exact_rough_event(dirs[i], normals[i], case.alpha, n1[i], n2[i], draws[i, 0], draws[i, 1],
                                               draws[i, 2], trig=trig) for i in range(len(dirs))]
    return _ROUGH_CACHE[key]


# ---- the phase cases -------------------------------------------------------------------------------------------------------
def hg_values(g, mu):
    return (1.0 - g * g) / (1.0 + g * g - 2.0 * g * mu) ** 1.5


def _tables():
    a5 = [0.0, 45.0, 90.0, 135.0, 180.0]
    a1801 = np.linspace(0.0, 180.0, 1801)
    mu1801 = np.cos(np.radians(a1801))
    a91 = np.linspace(0.0, 180.0, 91)
    c5 = np.cos(np.radians(a5))
    return {
        "constant": lambda: PhaseFunctionTable(a5, [1.0] * 5),
        "rayleigh": lambda: PhaseFunctionTable(a91, 1.0 + np.cos(np.radians(a91)) ** 2),
        "hg0.9-1801": lambda: PhaseFunctionTable(a1801, hg_values(0.9, mu1801)),
        "two-point": lambda: PhaseFunctionTable([0.0, 180.0], [1.0, 3.0]),
        # zero-mass segments at the start, in the middle and at the end of the mu axis
        "zero-mass": lambda: PhaseFunctionTable([0.0, 20.0, 50.0, 80.0, 110.0, 140.0, 160.0, 180.0],
                                                [0.0, 0.0, 1.0, 0.0, 0.0, 2.0, 0.0, 0.0]),
        # the first mu segment, [-1, 0], has mass 2e-300 of the whole (C_1 = 2e-300)
        "tiny-mass": lambda: PhaseFunctionTable([0.0, 90.0, 180.0], [1.0, 2e-300, 0.0]),
        "two-row-unit": lambda: PhaseFunctionTable(a5, np.vstack([1.0 + 0.8 * c5, 1.0 - 0.5 * c5]), wavelength=[1.0, 2.0]),
        "two-row": lambda: PhaseFunctionTable(a5, np.vstack([1.0 + 0.8 * c5, 1.0 - 0.5 * c5]), wavelength=[500.0, 600.0]),
        "five-row": lambda: PhaseFunctionTable(a5, np.vstack([1.0 + g * c5 for g in (0.5, 0.25, 0.0, -0.25, -0.5)]),
                                               wavelength=[450.0, 500.0, 575.0, 610.0, 720.0]),
        # 1801 x 20: its CDF alone is larger than a workgroup's LDS, so it is read from global memory
        "hg-1801x20": lambda: PhaseFunctionTable(a1801, hg_values(np.linspace(0.2, 0.9, 20)[:, None], mu1801[None, :]),
                                                 wavelength=np.linspace(400.0, 800.0, 20)),
    }


TABLES = _tables()


class PhaseCase:
    """A 2 x 2 x 2 block of n = 1 with one table component, rays started inside it.  component: "scatterer" or
    "luminophore"; container: "box", "mesh" (12 triangles) or "wide" (the box with 65 recorders).  Which kernel path a
    case reaches follows from `choose_variant` and `plan_lds` of pvt_trace.hip and the turn's call site in
    pvt_trace_kernel.h (`if constexpr (MESH || SEENW == 1)` calls phase_table_turn_call, else the turn is inlined):
    SEENW is 1 for a scene of at most 64 recorders and 4 beyond, MESH is set by a scene with a mesh, and the tables are
    staged in LDS when they fit a workgroup's budget (the 1801 x 20 CDF, 288 KB, cannot)."""

    def __init__(self, name, table, wavelengths=(555.0,), component="scatterer", container="box", seed=1, n=1000,
                 special=None):
        self.name, self.table_key, self.wavelengths, self.component = name, table, wavelengths, component
        self.container, self.seed, self.n, self.special = container, seed, n, special

    def __repr__(self):
        return self.name

    @functools.cached_property
    def table(self):
        table = TABLES[self.table_key]()
        if self.special == "on-a-knot":   # C_3 = C_4 (the zero-mass segment in the middle) := the nearest u2 of a ray
            u2 = self.phase_draws()[:, 0]
            at = int(np.argmin(np.abs(u2 - table.cdf[0, 3])))
            assert table.cdf[0, 3] == table.cdf[0, 4] and table.cdf[0, 2] < u2[at] < table.cdf[0, 5]
            table.cdf[0, 3] = table.cdf[0, 4] = u2[at]
            self.on_knot = at
        return table

    def phase_draws(self):
        """The draws of every ray from position 3 of its stream on (u1, u2, u3 of a table of several rows; u2, u3 of
        one row): tests/test_phase_turn_exact.py says why 3."""
        from oracle import oracle as O
        return np.array([O.uniforms(SEED + i, 6)[3:] for i in range(self.n)])

    def scene(self, tabled=True):
        """(scene, block); tabled=False: the same scene with the default isotropic phase function (the anchors)."""
        from pvtrace_amd.engine import Recorder
        from tests.law_cases import EMS_X, EMS_Y
        kw = dict(phase_function=self.table) if tabled else {}
        if self.component == "luminophore":
            comp = Luminophore(5.0, emission=np.column_stack((EMS_X, EMS_Y)), quantum_yield=1.0, name="dye", **kw)
        else:
            comp = Scatterer(5.0, quantum_yield=1.0, name="mist", **kw)
        world = Node(name="world", geometry=Box((64.0, 64.0, 64.0), material=Material(refractive_index=1.0)))
        material = Material(refractive_index=1.0, components=[comp])
        size = (2.0, 2.0, 2.0)
        geometry = Mesh.box(size, material=material) if self.container == "mesh" else Box(size, material=material)
        block = Node(name="block", parent=world, geometry=geometry)
        if self.container == "wide":
            block.recorders = [Recorder(f"r{i}", event="entering") for i in range(65)]
        return Scene(world), block

    def rays(self):
        """(positions, directions, wavelengths).  Every eighth ray runs along exactly +-x, +-y, +-z or has dz = -0.0 or
        +0.0; the others are random over the sphere."""
        rng = np.random.default_rng(self.seed)
        n = self.n
        pos = rng.uniform(-0.9, 0.9, (n, 3))
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        special = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0),
                   (0.6, 0.8, -0.0), (-0.8, 0.6, 0.0), (-1.0, -0.0, -0.0), (0.0, -0.0, -1.0)]
        for i in range(0, n, 8):
            v[i] = special[(i // 8) % len(special)]
        wl = np.asarray(self.wavelengths, dtype=np.float64)[rng.integers(0, len(self.wavelengths), n)]
        if self.special == "on-the-pick":   # 1 + u1 wherever that is a double (u1 a multiple of 2^-52): t = u1 exactly
            u1 = self.phase_draws()[:, 0]
            wl = np.where((1.0 + u1) - 1.0 == u1, 1.0 + u1, wl)
        return pos, np.ascontiguousarray(v), wl


# case                      table        turn      table memory   (kernel path; see PhaseCase)
PHASE_CASES = [
    PhaseCase("P-constant", "constant", seed=1),                                         # called    LDS
    PhaseCase("P-rayleigh", "rayleigh", seed=2),                                         # called    LDS
    PhaseCase("P-hg0.9-1801", "hg0.9-1801", seed=3),                                     # called    LDS
    PhaseCase("P-two-point", "two-point", seed=4),                                       # called    LDS
    PhaseCase("P-zero-mass", "zero-mass", seed=5),                                       # called    LDS
    PhaseCase("P-tiny-mass", "tiny-mass", seed=6),                                       # called    LDS
    # on a row (500, 600), below (400) and above (800) the range, between the rows (530, 580)
    PhaseCase("P-two-row", "two-row", wavelengths=(400.0, 500.0, 530.0, 580.0, 600.0, 800.0), seed=7),   # called LDS
    PhaseCase("P-five-row", "five-row", wavelengths=(300.0, 450.0, 470.0, 575.0, 590.0, 600.0, 700.0, 720.0, 900.0),
              seed=8, n=1500),                                                                   # called    LDS
    PhaseCase("P-hg-1801x20-global", "hg-1801x20", wavelengths=(390.0, 400.0 + 7 * 400.0 / 19, 555.0, 810.0),
              seed=9),                                                                   # called    global memory
    PhaseCase("P-two-row-wide-inlined", "two-row", wavelengths=(400.0, 530.0, 580.0, 800.0), container="wide",
              seed=10),                                                                  # INLINED   LDS
    PhaseCase("P-two-row-mesh", "two-row", wavelengths=(500.0, 530.0, 580.0, 600.0), container="mesh", seed=11),  # called (MESH) LDS
    PhaseCase("P-rayleigh-luminophore", "rayleigh", component="luminophore", seed=12),   # called    LDS, EMIT
    PhaseCase("P-two-row-on-the-pick", "two-row-unit", wavelengths=(1.5,), special="on-the-pick", seed=13),   # called LDS
    PhaseCase("P-zero-mass-on-a-knot", "zero-mass", special="on-a-knot", seed=14),       # called    LDS
]
PHASE_BY_NAME = {c.name: c for c in PHASE_CASES}

_PHASE_CACHE = {}


def phase_refs(case, dirs, wl, u1, u2, u3, trig):
    """`exact_phase_turn` of every ray of a case, computed once per (case, draws, trig)."""
    key = (case.name, trig, np.asarray(u2).tobytes(), np.asarray(u3).tobytes(), None if u1 is None else np.asarray(u1).tobytes())
    if key not in _PHASE_CACHE:
        _PHASE_CACHE[key] = [exact_phase_turn(case.table, wl[i], dirs[i], 0.0 if u1 is None else u1[i], u2[i], u3[i],
                                              trig=trig) for i in range(len(dirs))]
    return _PHASE_CACHE[key]
