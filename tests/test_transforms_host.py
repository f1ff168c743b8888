"""Host side of quflow_amd.transforms (no GPU needed), and the independent evaluator of the synthesis that the device tests
(tests/test_hip_sht.py) compare against.

* shr2shc, shc2shr, sphgrid, fun2img, img2fun against tests/golden/transforms.npz, made by the reference itself
  (tools/gen_transforms_golden.py) on inputs rebuilt here from integer hashes; the outputs must match bit for bit (SHA-256
  of their bytes), and the argument rules of the reference.
* The evaluator: f = sqrt(4 pi) sum w_l a_lm Y_lm on the MW grid in np.longdouble.  lambda_lm(theta) comes from the
  normalised three-term recurrence in l, vectorised over rings, with an explicit binary exponent per ring (np.frexp /
  np.ldexp) so that sin^m theta at m = 8191 (~1e-30000, below even the long double range) is carried exactly; the ring
  transform is an explicit DFT.  It is pinned here to scipy.special.sph_harm_y for every (l, m) at L <= 24 and to the three
  l = 1 closed forms.  Its own error is that of long double arithmetic (~1e-19 relative per operation), far below fp64.
* The same evaluator at large L (tests/test_hip_sht_large.py): legendre_sums walks the recurrence once over l with every
  order m (or a chosen few) and every chosen ring vectorised, O(L^2) per ring, and reproduces synth_ref's Legendre sums
  bit for bit; synth_rings does the ring transform in fp64 column blocks and reports its own rounding bound.
* Rings: theta_t = pi q_t with q_t = (2t+1)/(2L-1) ROUNDED TO FLOAT64, the argument the device hands to sincospi; the
  evaluator then sees the same sample points as the device and differs from it only by arithmetic.
"""
import hashlib
import os

import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import transforms as T

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transforms.npz")
LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")
FOURPI = 4 * PI


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator
# ---------------------------------------------------------------------------------------------------------------------

def ring_q(L):
    """q_t = (2t+1)/(2L-1) as float64: theta_t = pi q_t."""
    return (2.0 * np.arange(L) + 1.0) / (2.0 * L - 1.0)


def cospi_sinpi(q):
    """cos(pi q), sin(pi q) in long double with sincospi's exact reduction: sin(pi q) = sin(pi (1 - q)) with 1 - q exact,
    so that the south pole q = 1 has sin = 0 exactly (long double pi is not pi: sin(PI) is ~5e-20)."""
    q = np.asarray(q, dtype=np.float64).astype(LD)
    upper = q > 0.5
    r = np.where(upper, 1 - q, q)
    return np.where(upper, -np.cos(PI * r), np.cos(PI * r)), np.sin(PI * r)


def berezin_ld(L):
    """w_l = sqrt(prod_{j=1..l} (L-j)/(L+j)) in long double: what berezin_multipliers(L) (utils.py:108-135) computes
    through log-gamma."""
    w2 = np.ones(L, dtype=LD)
    for el in range(1, L):
        w2[el] = w2[el - 1] * (LD(L - el) / LD(L + el))
    return np.sqrt(w2)


def lambda_iter(m, q):
    """Yields (l, mantissa, exponent) for l = m, m+1, ...: lambda_lm(pi q_t) = mantissa * 2**exponent at every ring
    (arrays over q), long double mantissa renormalised at every degree."""
    x, s = cospi_sinpi(q)
    sm, se = np.frexp(s)
    prod = LD(1)
    for k in range(1, m + 1):
        prod *= LD(2 * k - 1) / LD(2 * k)
    c = np.sqrt(LD(2 * m + 1) / FOURPI * prod) * (-1 if m % 2 else 1)
    p1, d = np.frexp(sm ** m)            # sin^m = sm^m 2^(m se); sm^m >= 2^-m stays in range
    E = se.astype(np.int64) * m + d
    p1 = p1 * c
    p2 = np.zeros_like(p1)
    el = m
    yield el, p1, E
    while True:
        el += 1
        a = np.sqrt(LD(4 * el * el - 1) / LD((el - m) * (el + m)))
        b = np.sqrt(LD((el - 1 - m) * (el - 1 + m)) / LD(4 * (el - 1) * (el - 1) - 1))
        p = a * (x * p1 - b * p2)
        mant, d = np.frexp(p)
        p2 = np.ldexp(p1, -d)
        p1 = mant
        E = E + d
        yield el, p1, E


def lambda_rows(m, lmax, q):
    """lambda_lm(theta_t) for l = m..lmax (rows) at the rings q (columns), long double (values below its range are 0)."""
    out = np.empty((lmax - m + 1, len(q)), dtype=LD)
    for el, mant, E in lambda_iter(m, q):
        if el > lmax:
            break
        out[el - m] = np.ldexp(mant, E)
    return out


def lambda_at(el, m, q):
    """lambda_lm at the rings q as (mantissa, exponent): exact far below every floating-point range."""
    for ell, mant, E in lambda_iter(m, q):
        if ell == el:
            return mant, E


def padded(omega, L):
    om = np.zeros(L * L, dtype=np.clongdouble)
    n = min(len(omega), L * L)
    om[:n] = np.asarray(omega)[:n]
    return om


def legendre_ref(omega, L, berezin):
    """synth_ref's Legendre stage, every order at every ring: (G+, G-) as (L, L) [m, t] arrays."""
    a = padded(omega, L)
    w = berezin_ld(L) if berezin else np.ones(L, dtype=LD)
    el = np.floor(np.sqrt(np.arange(L * L))).astype(np.int64)
    a = a * (np.sqrt(FOURPI) * w[el])
    q = ring_q(L)
    Gp = np.zeros((L, L), dtype=np.clongdouble)     # [m, t]: sum_l a_lm lambda_lm
    Gm = np.zeros((L, L), dtype=np.clongdouble)     # [m, t]: sum_l a_l,-m lambda_l,-m,  lambda_l,-m = (-1)^m lambda_lm
    for m in range(L):
        lam = lambda_rows(m, L - 1, q)
        ls = np.arange(m, L)
        Gp[m] = a[ls * ls + ls + m] @ lam
        if m > 0:
            Gm[m] = ((-1) ** m * a[ls * ls + ls - m]) @ lam
    return Gp, Gm


def synth_ref(omega, L, isreal, berezin):
    """shc2fun(omega, isreal, N=L, berezin) in long double: (L, 2L-1) real (isreal) or complex."""
    Gp, Gm = legendre_ref(omega, L, berezin)
    P = 2 * L - 1
    k = (np.arange(L)[:, None] * np.arange(P)[None, :]) % P          # exact reduction of m p mod (2L-1)
    ang = 2 * PI * k.astype(LD) / P
    cs, sn = np.cos(ang), np.sin(ang)
    if isreal:
        # f = sum_l Re(a_l0) lambda_l0 + 2 sum_{m>0} Re(G_m e^{i m phi})
        wm = np.full(L, 2, dtype=LD)
        wm[0] = 1
        return (wm[:, None] * Gp.real).T @ cs - (wm[:, None] * Gp.imag).T @ sn
    e = cs + 1j * sn
    return Gp.T @ e + Gm.T @ np.conj(e)


def real_term(el, m, a, L, rows=None, cols=None):
    """The contribution w_m Re(a lambda_lm(theta_t) e^{i m phi_p}) (w_0 = 1, w_m = 2) of ONE complex coefficient a_lm,
    m >= 0, to a real synthesis (berezin=False), at the rings `rows` x the columns `cols`; also its scale per ring,
    w_m |a| (lambda_lm^2 + lambda_l-1,m^2)^(1/2): the size of the pair a recurrence in l carries, which its rounding errors
    are relative to (lambda_lm alone passes through zero between rings in the oscillatory region).  Long double."""
    P = 2 * L - 1
    rows = np.arange(L) if rows is None else np.asarray(rows)
    cols = np.arange(P) if cols is None else np.asarray(cols)
    prev = np.zeros(len(rows), dtype=LD)
    for ell, mant, E in lambda_iter(m, ring_q(L)[rows]):
        lam = np.ldexp(mant, E)
        if ell == el:
            break
        prev = lam
    ang = 2 * PI * ((m * cols) % P).astype(LD) / P
    w = LD(1 if m == 0 else 2)
    av = np.clongdouble(a) * np.sqrt(FOURPI)
    val = w * (av.real * np.outer(lam, np.cos(ang)) - av.imag * np.outer(lam, np.sin(ang)))
    return val, w * abs(av) * np.sqrt(lam * lam + prev * prev)


# ---- the evaluator at large L: O(L^2) work per ring instead of synth_ref's O(L^3) for the whole grid

def _workers():
    """Threads for the evaluator (numpy releases the GIL inside its long double loops): at most 16."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(16, n))


def legendre_walk(L, q, ms):
    """The recurrence in l at the rings q for the orders ms (sorted), vectorised over both: yields (l, k, cur, prev, E),
    where the first k rows (the orders ms[:k] <= l) hold lambda_{l,ms[i]} = cur 2^E and lambda_{l-1,ms[i]} = prev 2^E (the
    arrays are reused from one degree to the next).  The operations are lambda_iter's; the pair is renormalised every
    16 degrees instead of at every one, which changes no value (a power-of-two scale passes exactly through the
    recurrence), so cur 2^E is the same bits as lambda_iter's value wherever it is a normal long double."""
    x, s = cospi_sinpi(q)
    sm, se = np.frexp(s)
    se = se.astype(np.int64)
    R, n = len(q), len(ms)
    kk = np.arange(1, int(ms[-1]) + 1, dtype=np.int64)
    prod = np.cumprod(np.concatenate([[LD(1)], (2 * kk - 1).astype(LD) / (2 * kk).astype(LD)]))
    c = np.sqrt((2 * ms + 1).astype(LD) / FOURPI * prod[ms])
    c[ms % 2 == 1] *= -1
    cur = np.zeros((n, R), dtype=LD)
    prev = np.zeros((n, R), dtype=LD)
    E = np.zeros((n, R), dtype=np.int64)
    tmp = np.empty((n, R), dtype=LD)
    k = 0
    for el in range(int(ms[0]), L):
        if k:
            m = ms[:k]
            a = np.sqrt(LD(4 * el * el - 1) / ((el - m) * (el + m)).astype(LD))
            b = np.sqrt(((el - 1 - m) * (el - 1 + m)).astype(LD) / LD(4 * (el - 1) * (el - 1) - 1))
            np.multiply(x, cur[:k], out=tmp[:k])
            tmp[:k] -= b[:, None] * prev[:k]
            np.multiply(a[:, None], tmp[:k], out=prev[:k])
            cur, prev = prev, cur
            if el % 16 == 0:
                mant, d = np.frexp(cur[:k])
                prev[:k] = np.ldexp(prev[:k], -d)
                cur[:k] = mant
                E[:k] += d
        if k < n and ms[k] == el:
            mant, d = np.frexp(sm ** el)
            cur[k] = mant * c[k]
            prev[k] = 0
            E[k] = se * el + d
            k += 1
        yield el, k, cur, prev, E


def _legendre_pass(sets, L, q, ms):
    """legendre_sums at the rings q: one walk shared by every coefficient set."""
    R, n = len(q), len(ms)
    F = np.zeros((n, R), dtype=LD)                   # 2^E, refreshed when E changes
    prev64 = np.zeros((n, R))                        # lambda_{l-1,m} in fp64, for the scale
    wm = np.where(ms == 0, 1.0, 2.0)
    acc = []
    for _, _, ng in sets:
        z = lambda: np.zeros((n, R), dtype=LD)       # noqa: E731
        acc.append([z(), z(), z() if ng else None, z() if ng else None, np.zeros(R)])
    k0 = 0
    for el, k, cur, prev, E in legendre_walk(L, q, ms):
        if el % 16 == 0:
            F[:k] = np.ldexp(LD(1), E[:k])
        elif k > k0:
            F[k0:k] = np.ldexp(LD(1), E[k0:k])
            prev64[k0:k] = 0
        k0 = k
        lam = cur[:k] * F[:k]
        lam64 = lam.astype(np.float64)
        rho = np.hypot(lam64, prev64[:k])
        prev64[:k] = lam64
        mk = ms[:k]
        for (co, sc, ng), (gp_r, gp_i, gm_r, gm_i, scale) in zip(sets, acc):
            row = co[el * el + el + mk]
            ar, ai = row.real.astype(LD) * sc[el], row.imag.astype(LD) * sc[el]
            gp_r[:k] += ar[:, None] * lam
            gp_i[:k] += ai[:, None] * lam
            wa = np.abs(row) * float(sc[el])
            if ng:
                row = np.where(mk % 2 == 1, -1, 1) * np.where(mk > 0, co[el * el + el - mk], 0)
                br, bi = row.real.astype(LD) * sc[el], row.imag.astype(LD) * sc[el]
                gm_r[:k] += br[:, None] * lam
                gm_i[:k] += bi[:, None] * lam
                wa = wa + np.abs(row) * float(sc[el])
            else:
                wa = wa * wm[:k]
            scale += wa @ rho
    return [(gr + 1j * gi, None if hr is None else hr + 1j * hi, scale) for gr, gi, hr, hi, scale in acc]


def legendre_sums(a, L, rings, neg=False, scale_l=None, ms=None):
    """The Legendre stage in long double at the rings `rings` (rows: the orders ms, default every m < L):
        G+[m, r] = sum_l a~_lm lambda_lm(theta_r),   a~_lm = scale_l[l] a_lm  (scale_l = sqrt(4 pi) w_l, default sqrt(4 pi)),
    and with `neg` (a complex synthesis) also G-[m, r] = sum_l (-1)^m a~_l,-m lambda_lm (0 at m = 0).  Also the per-ring
    scale the recurrence's rounding errors are relative to (real_term's, summed):
        scale[r] = sum_{m, l} w_m |a~_lm| (lambda_lm^2 + lambda_l-1,m^2)^(1/2),   w_0 = 1, w_m = 2  (real synthesis),
        scale[r] = sum_{m, l} (|a~_lm| + |a~_l,-m|) (lambda_lm^2 + lambda_l-1,m^2)^(1/2)   (neg: both accumulators),
    in fp64 (terms below the fp64 range, far below the bar's 1e-300 floor, are dropped: it only sizes a bar).  Returns
    (G+, G- or None, scale).  `a` is an array of complex coefficients (trimmed or zero-padded to L^2) or a list of them,
    scale_l and neg then per entry or shared: the sets share one walk of the recurrence.  Loops over l with all active m
    vectorised; ~L^2 |rings| / 2 steps (for all m), spread over threads by rings."""
    single = not isinstance(a, (list, tuple))
    a = [a] if single else list(a)
    scale_l = scale_l if isinstance(scale_l, (list, tuple)) else [scale_l] * len(a)
    neg = neg if isinstance(neg, (list, tuple)) else [neg] * len(a)
    sets = []
    for om, sc, ng in zip(a, scale_l, neg):
        om = np.asarray(om)
        co = np.zeros(L * L, dtype=np.complex128)
        co[:min(len(om), L * L)] = om[:L * L]
        sc = np.full(L, np.sqrt(FOURPI), dtype=LD) if sc is None else np.asarray(sc, dtype=LD)
        sets.append((co, sc, bool(ng)))
    ms = np.arange(L, dtype=np.int64) if ms is None else np.asarray(ms, dtype=np.int64)
    assert np.all(np.diff(ms) > 0) and 0 <= ms[0] and ms[-1] < L
    rings = np.asarray(rings, dtype=np.int64)
    q = ring_q(L)[rings]
    nw = min(_workers(), max(1, len(rings) // 2))
    parts = np.array_split(np.arange(len(rings)), nw)
    if nw == 1:
        outs = [_legendre_pass(sets, L, q, ms)]
    else:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(nw) as ex:
            outs = list(ex.map(lambda ix: _legendre_pass(sets, L, q[ix], ms), parts))
    res = []
    for i in range(len(sets)):
        gp = np.concatenate([o[i][0] for o in outs], axis=1)
        gm = None if outs[0][i][1] is None else np.concatenate([o[i][1] for o in outs], axis=1)
        res.append((gp, gm, np.concatenate([o[i][2] for o in outs])))
    return res[0] if single else res


def twiddles(L):
    """(cos, sin)(2 pi k/(2L-1)), k < 2L-1, in long double rounded once to float64 (the argument reduced to (-1, 1] half
    turns, as on the device): each within eps/2 of the exact value."""
    P = 2 * L - 1
    k = np.arange(P, dtype=np.int64)
    j = np.where(2 * k > P, k - P, k).astype(LD)
    ang = 2 * PI * j / P
    return np.cos(ang).astype(np.float64), np.sin(ang).astype(np.float64)


def synth_rings(Gp, Gm, L, isreal, cols=None, ms=None, block=512):
    """The ring transform of legendre_sums' output: f[r, p] at the rings of G and the columns `cols` (default all 2L-1),
    rows of G the orders `ms` (default 0..L-1).  Real (isreal, w_0 = 1, w_m = 2, Gm unused):
        f = sum_m w_m (Re G+_m cos(m phi) - Im G+_m sin(m phi));
    complex: f = sum_m G+_m e^{i m phi} + G-_m e^{-i m phi}.
    fp64 (BLAS) on G rounded to fp64 and twiddles at the exact reduction (m p) mod (2L-1), in column blocks: no
    L x (2L-1) table is formed.  Returns (f, err) with err[r] = (2 n + 4) eps sum_m w_m (|G+_m| + |G-_m|), n the number of
    orders: a bound on this step's own rounding (n products of two terms per point, each of G, the twiddle and the product
    rounded once, summed in any order)."""
    P = 2 * L - 1
    ms = np.arange(L, dtype=np.int64) if ms is None else np.asarray(ms, dtype=np.int64)
    cols = np.arange(P, dtype=np.int64) if cols is None else np.asarray(cols, dtype=np.int64)
    cs, sn = twiddles(L)
    eps = np.finfo(np.float64).eps
    if isreal:
        w = np.where(ms == 0, 1, 2).astype(LD)[:, None]
        Ar = np.concatenate([w * Gp.real, -w * Gp.imag]).astype(np.float64)
        Ai = None
        mag = (w * np.abs(Gp)).sum(axis=0)
    else:
        gm = np.zeros_like(Gp) if Gm is None else Gm
        Ar = np.concatenate([Gp.real + gm.real, gm.imag - Gp.imag]).astype(np.float64)
        Ai = np.concatenate([Gp.imag + gm.imag, Gp.real - gm.real]).astype(np.float64)
        mag = (np.abs(Gp) + np.abs(gm)).sum(axis=0)
    R = Gp.shape[1]
    f = np.empty((R, len(cols)), dtype=np.float64 if isreal else np.complex128)
    for c0 in range(0, len(cols), block):
        cc = cols[c0:c0 + block]
        k = (ms[:, None] * cc[None, :]) % P
        Tw = np.concatenate([cs[k], sn[k]])
        if isreal:
            f[:, c0:c0 + block] = Ar.T @ Tw
        else:
            f[:, c0:c0 + block] = Ar.T @ Tw + 1j * (Ai.T @ Tw)
    err = (2 * len(ms) + 4) * eps * mag.astype(np.float64)
    return f, err


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator against independent references
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 2, 7, 24])
def test_evaluator_legendre_vs_scipy(L):
    from scipy.special import sph_harm_y
    q = ring_q(L)
    theta = np.pi * q
    for m in range(L):
        lam = lambda_rows(m, L - 1, q).astype(np.float64)
        for el in range(m, L):
            Y = sph_harm_y(el, m, theta, 0.0)
            np.testing.assert_allclose(lam[el - m], Y.real, rtol=0, atol=1e-13, err_msg="(l, m) = (%d, %d)" % (el, m))


@pytest.mark.parametrize("L", [3, 24])
def test_evaluator_synthesis_vs_scipy(L):
    """Every unit coefficient (l, m), -l <= m <= l, synthesised by the evaluator equals sqrt(4 pi) Y_lm on the grid."""
    from scipy.special import sph_harm_y
    theta, phi = T.sphgrid(L)
    for ind in range(L * L):
        el = int(np.floor(np.sqrt(ind)))
        m = ind - el * el - el
        om = np.zeros(L * L, dtype=complex)
        om[ind] = 1.0
        f = synth_ref(om, L, isreal=False, berezin=False)
        Y = np.sqrt(4 * np.pi) * sph_harm_y(el, m, theta, phi)
        np.testing.assert_allclose(f.astype(np.complex128), Y, rtol=0, atol=1e-12, err_msg="(l, m) = (%d, %d)" % (el, m))


def test_evaluator_l1_closed_forms():
    """Unit shr coefficients at l = 1 (berezin=False): sqrt(3) cos(theta), sqrt(3) sin(theta) cos(phi),
    -sqrt(3) sin(theta) sin(phi) for m = 0, 1, -1."""
    L = 5
    theta = PI * ring_q(L).astype(LD)
    phi = 2 * PI * np.arange(2 * L - 1).astype(LD) / (2 * L - 1)
    th, ph = np.meshgrid(theta, phi, indexing="ij")
    r3 = np.sqrt(LD(3))
    want = {0: r3 * np.cos(th), 1: r3 * np.sin(th) * np.cos(ph), -1: -r3 * np.sin(th) * np.sin(ph)}
    for m, w in want.items():
        om = np.zeros(L * L)
        om[qfa.elm2ind(1, m)] = 1.0
        # (bar: shr2shc's float64 factor 1/sqrt(2) carries one rounding, 1.1e-16 relative)
        f = synth_ref(T.shr2shc(om), L, isreal=True, berezin=False)
        assert np.abs(f - w).max() < 1e-15, (m, float(np.abs(f - w).max()))
        # the complex synthesis of the same (real) function agrees and is real
        fc = synth_ref(T.shr2shc(om), L, isreal=False, berezin=False)
        assert np.abs(fc.real - w).max() < 1e-15 and np.abs(fc.imag).max() < 1e-15, m


def test_evaluator_tracks_exponents_below_every_range():
    """lambda_{L-1,L-1} at the first ring for L = 8192 is ~1e-30000: the mantissa / exponent pair holds it exactly (its
    log10 matches the closed form log10|c_m| + m log10 sin(theta)), where the value itself would be 0."""
    L = 8192
    m = L - 1
    q = ring_q(L)[:1]
    mant, E = lambda_at(m, m, q)
    log10 = np.log10(np.abs(mant.astype(np.float64))) + E * np.log10(2.0)
    prod = np.exp(np.sum(np.log(np.arange(1, 2 * m, 2, dtype=np.float64)) - np.log(np.arange(2, 2 * m + 1, 2, dtype=np.float64))))
    want = 0.5 * np.log10((2 * m + 1) / (4 * np.pi) * prod) + m * np.log10(np.sin(np.pi * q))
    assert abs(log10[0] - want[0]) < 1e-9 and log10[0] < -29000, (log10, want)
    assert np.ldexp(mant, E)[0] == 0


@pytest.mark.parametrize("L", [1, 2, 3, 24, 64])
def test_legendre_sums_are_synth_refs_sums(L):
    """legendre_sums (all orders, or a few) at every ring is synth_ref's Legendre stage bit for bit: the same operations
    on the same values, in the same order.  synth_rings then agrees with synth_ref within the bound it reports."""
    rng = np.random.default_rng(L)
    om = rng.standard_normal(L * L) + 1j * rng.standard_normal(L * L)
    sc = np.sqrt(FOURPI) * berezin_ld(L)
    Gpr, Gmr = legendre_ref(om, L, berezin=True)
    (Gp, Gm, scale), (Gr, none, scale_r) = legendre_sums([om, om], L, np.arange(L), neg=[True, False], scale_l=sc)
    assert np.array_equal(Gp, Gpr) and np.array_equal(Gm, Gmr) and np.array_equal(Gr, Gpr) and none is None
    ms = np.unique([0, L // 2, L - 1])
    Gq, Gmq, _ = legendre_sums(om, L, np.arange(L), neg=True, scale_l=sc, ms=ms)
    assert np.array_equal(Gq, Gpr[ms]) and np.array_equal(Gmq, Gmr[ms])
    # the scale bounds every accumulator: sum_m w_m |G+_m| (real), sum_m |G+_m| + |G-_m| (complex)
    w = np.where(np.arange(L) == 0, 1, 2)[:, None]
    assert np.all((w * np.abs(Gpr)).sum(axis=0).astype(float) <= scale_r * (1 + 1e-12))
    assert np.all((np.abs(Gpr) + np.abs(Gmr)).sum(axis=0).astype(float) <= scale * (1 + 1e-12))
    for isreal in (True, False):
        f, err = synth_rings(Gp, Gm, L, isreal)
        ref = synth_ref(om, L, isreal, berezin=True)
        assert np.all(np.abs(f - ref) <= err[:, None] + 1e-300), isreal
        cols = np.array([0, L // 2, 2 * L - 2])
        fc, _ = synth_rings(Gq, Gmq, L, isreal, cols=cols, ms=ms)
        fq, _ = synth_rings(Gpr[ms], Gmr[ms], L, isreal, ms=ms)
        assert np.array_equal(fc, fq[:, cols]), isreal


def test_legendre_sums_agree_with_synth_ref_at_300():
    """L = 300 on sampled rings, both routes, against the O(L^3) evaluator: within synth_rings' own fp64 bound plus the
    long double rounding of the sums (L eps_ld relative to the scale)."""
    L = 300
    rng = np.random.default_rng(300)
    om = rng.standard_normal(L * L) + 1j * rng.standard_normal(L * L)
    om /= np.linalg.norm(om)
    rings = np.array([0, 1, 2, 63, 64, 149, 150, 255, 256, 297, 298, 299])
    Gp, Gm, scale = legendre_sums(om, L, rings, neg=True)
    eps_ld = float(np.finfo(LD).eps)
    for isreal in (True, False):
        f, err = synth_rings(Gp, Gm, L, isreal)
        ref = synth_ref(om, L, isreal, berezin=False)[rings]
        assert np.all(np.abs(f - ref) <= err[:, None] + 4 * L * eps_ld * scale[:, None]), isreal


def test_legendre_walk_tracks_exponents_below_every_range():
    """At L = 8192 and the first ring, the all-orders walk ends at l = L-1 with the mantissa and exponent of lambda_iter
    for every sampled order, lambda_{L-1,L-1} (~1e-30000) included."""
    L = 8192
    q = ring_q(L)[:1]
    for el, k, cur, prev, E in legendre_walk(L, q, np.arange(L, dtype=np.int64)):
        pass
    assert el == L - 1 and k == L
    mant, d = np.frexp(cur[:, 0])
    E = E[:, 0] + d
    for m in (0, 1, 2, 255, 4096, L - 2, L - 1):
        want_mant, want_E = lambda_at(L - 1, m, q)
        want_mant, d = np.frexp(want_mant)      # (lambda_iter leaves the seed's mantissa unnormalised)
        assert mant[m] == want_mant[0] and E[m] == want_E[0] + d[0], m
    assert E[L - 1] < -99000


@pytest.mark.parametrize("L", [16, 300, 512])
def test_berezin_product_is_the_reference_multiplier(L):
    """The long double product the device uses for w_l equals berezin_multipliers(L) (the reference's log-gamma form) to
    that form's own rounding: ~|lgamma| eps relative."""
    w_ref = qfa.berezin_multipliers(L)
    el = np.floor(np.sqrt(np.arange(L * L))).astype(int)
    w = berezin_ld(L)[el].astype(np.float64)
    big = w_ref > 1e-200
    rel = np.abs(w[big] - w_ref[big]) / w_ref[big]
    assert rel.max() < 1e-12, rel.max()


# ---------------------------------------------------------------------------------------------------------------------
# host transforms against the reference
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def det_values(n, salt):
    """The fixture's inputs, rebuilt bit for bit from integer hashes (as tools/gen_transforms_golden.py makes them)."""
    k = np.arange(n, dtype=np.int64)
    v = (k * 2654435761 + (salt + 1) * 40503) % 2147483647
    return (v / 2147483647.0 - 0.5) * 4.0


def det_image(shape, salt):
    k = np.arange(int(np.prod(shape)), dtype=np.int64)
    return ((k * 2654435761 + (salt + 1) * 40503) % 2147483647 % 256).astype(np.uint8).reshape(shape)


def expect(gold, key, got):
    """`got` is the reference's output `key` bit for bit: dtype, shape and the SHA-256 digest of its bytes (and the stored
    array itself where the fixture keeps it, for a readable difference)."""
    got = np.ascontiguousarray(got)
    if key in gold.files:
        np.testing.assert_array_equal(got, gold[key])
    assert str(got.dtype) == str(gold[key + "__dtype"]), key
    assert got.shape == tuple(gold[key + "__shape"]), key
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(gold[key + "__sha256"]), key


@pytest.mark.parametrize("N", [17, 128])
def test_shr2shc_shc2shr_vs_reference(gold, N):
    omr = det_values(N * N, 1)
    omc = det_values(N * N, 2) + 1j * det_values(N * N, 3)
    expect(gold, "shr2shc_%d" % N, T.shr2shc(omr))
    expect(gold, "shc2shr_%d" % N, T.shc2shr(omc))
    expect(gold, "shc2shr_shr2shc_%d" % N, T.shc2shr(T.shr2shc(omr)))
    expect(gold, "shr2shc_shc2shr_%d" % N, T.shr2shc(T.shc2shr(T.shr2shc(omr))))
    # the reference tests' round trips (quflow/tests/test_transforms.py:29-43)
    np.testing.assert_allclose(T.shc2shr(T.shr2shc(omr)), omr)
    c = T.shr2shc(omr)
    np.testing.assert_allclose(T.shr2shc(T.shc2shr(c)), c)


@pytest.mark.parametrize("n", [5, 12, 30])
def test_shr2shc_cut_short_lengths(gold, n):
    expect(gold, "shr2shc_n%d" % n, T.shr2shc(det_values(n, 6)))


@pytest.mark.parametrize("n", [0, 3, 7, 8, 13, 14, 31])
def test_shr2shc_lengths_the_reference_refuses(n):
    """The reference's loops index past a last degree cut short (IndexError) at exactly these lengths."""
    with pytest.raises(IndexError):
        T.shr2shc(np.ones(n))
    with pytest.raises(IndexError):
        T.shc2shr(np.ones(n, dtype=complex))


@pytest.mark.parametrize("N", [17, 128])
def test_sphgrid_fun2img_img2fun_vs_reference(gold, N):
    theta, phi = T.sphgrid(N)
    expect(gold, "sphgrid_theta_%d" % N, theta)
    expect(gold, "sphgrid_phi_%d" % N, phi)
    f = det_values(N * (2 * N - 1), 4).reshape(N, 2 * N - 1)
    expect(gold, "fun2img_%d" % N, T.fun2img(f))
    expect(gold, "fun2img_lim_%d" % N, T.fun2img(f, lim=(-0.5, 1.5)))
    expect(gold, "fun2img_sym_%d" % N, T.fun2img(f, lim=0.75))
    img = det_image((N, 2 * N - 1), 5)
    expect(gold, "img2fun_%d" % N, T.img2fun(img))
    expect(gold, "img2fun_lim_%d" % N, T.img2fun(img, lim=(-2.0, 3.0)))


def test_package_exports_transforms():
    for name in ("shr2fun", "shc2fun", "shr2shc", "shc2shr", "as_fun", "as_shr", "sphgrid", "fun2img", "img2fun",
                 "fun2shr", "fun2shc"):
        assert getattr(qfa, name) is getattr(T, name), name
    assert qfa.transforms is T


def test_analysis_is_refused_by_name():
    f = np.zeros((4, 7))
    with pytest.raises(NotImplementedError, match="fun2shr"):
        T.fun2shr(f)
    with pytest.raises(NotImplementedError, match="fun2shc"):
        T.fun2shc(f)
    with pytest.raises(NotImplementedError, match="fun2shr"):
        T.as_shr(f)
    with pytest.raises(NotImplementedError, match="fun2shr"):
        T.as_shr(np.zeros((4, 7), dtype=np.uint8))


def test_host_dispatch_branches():
    f = np.random.default_rng(0).standard_normal((4, 7))
    assert T.as_fun(f) is not None and np.array_equal(T.as_fun(f), f)
    img = np.arange(28, dtype=np.uint8).reshape(4, 7)
    np.testing.assert_array_equal(T.as_fun(img), T.img2fun(img))
    omr = np.random.default_rng(1).standard_normal(16)
    assert T.as_shr(omr) is omr or np.array_equal(T.as_shr(omr), omr)
    omc = T.shr2shc(omr)
    np.testing.assert_array_equal(T.as_shr(omc), T.shc2shr(omc))


def test_synthesis_argument_rules_on_the_host():
    """What is refused before any device work: a non-square length with N = -1 (the reference's assert), a bandwidth
    outside 1..8192, complex input to shr2fun."""
    with pytest.raises(AssertionError, match="right length"):
        T.shc2fun(np.ones(5, dtype=complex))
    with pytest.raises(AssertionError, match="right length"):
        T.shr2fun(np.ones(12))
    with pytest.raises(ValueError, match="outside 1..8192"):
        T.shc2fun(np.ones(4, dtype=complex), N=8193)
    with pytest.raises(ValueError, match="outside 1..8192"):
        T.shr2fun(np.ones(4), N=0)
    with pytest.raises(AssertionError, match="real"):
        T.shr2fun(np.ones(4, dtype=complex))
    with pytest.raises(IndexError):
        T.shr2fun(np.ones(7), N=3)
