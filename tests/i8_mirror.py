"""A numpy restatement of the arithmetic of quflow_amd/csrc/ozaki.hip (the complex128 product on the int8 matrix
cores by digit splitting), written from that file's comments and code: no GPU and no import of the library.

The kernels are exact integer arithmetic followed by a short, fixed sequence of IEEE operations, so what they store can
be predicted bit for bit:

  slice_rows       k_oz_slice<KD>: the row scale, the KD balanced base-128 digits, the prefix digit sums of the row record
  product          k_oz_gemm<KD, ., KDM>: offset-form U1 / U2 with their corrections, U3 from the byte-wise sum and
                   difference digits, one int32 group per a + b = s < KD, OZ_RESULT's conversion
  fused_epilogue   what FUSEDEPI stores: the mirrored T, comm, dW, Whalf, W_next, Whalf_step, the residual row sums

Operations a compiler may contract into an fma are noted where they occur; each of them multiplies by a power of two or
an integer below 2^31 by a power of two, so the product is exact and the contraction changes no bit (as long as no
intermediate is subnormal: the tests keep scales' products normal).

`perturb` arguments exist for tests/test_i8_mirror_host.py only: each makes the mirror wrong in one low-order way.
"""
import numpy as np

TILE = 64
SMALLEST_NORMAL_EXP = -1022


def _row_exponent(m):
    """k_oz_slice's scale rule for the row maxima m (finite, >= 0): e with s = 2^e the smallest power of two such that
    m / s <= 63/128; e = 0 for a zero row and for m >= 1e300 (the kernel's guard)."""
    f, e = np.frexp(m)                              # m = f 2^e, f in [0.5, 1)
    e = e + np.where(f <= 0.984375, 1, 2)
    return np.where((m > 0.0) & (m < 1e300), e, 0).astype(np.int64)


def slice_rows(X, KD, perturb=None):
    """Row i of the complex matrix X cut as k_oz_slice<KD> cuts it.  Returns a dict:
         s      [N]         the row scales (doubles, powers of two; NaN for a row with a non-finite entry)
         dr, di [KD, N, N]  the balanced digits d_t in [-64, 63] of Re X / s and Im X / s (int64)
         sums   [2, KD, N]  sums[c][t][i] = sum_{u <= t} sum_k d_u(i, k): the prefix digit sums of the row record
       Two edge rules:
         * a row whose scale would fall below the smallest normal power of two (1 / s overflows) is flushed: zero digits, s = 1;
         * a row with an inf or a NaN in it gets the scale NaN (its digits do not matter: zero here)."""
    X = np.ascontiguousarray(X, dtype=np.complex128)
    N = X.shape[0]
    v = X.view(np.float64).reshape(N, N, 2)
    a = np.abs(v).reshape(N, -1)
    bad = ~np.all(np.isfinite(a), axis=1)
    m = np.where(bad, 0.0, np.fmax.reduce(np.where(np.isnan(a), 0.0, a), axis=1))
    e = _row_exponent(m)
    flush = e < SMALLEST_NORMAL_EXP
    e = np.where(flush, 0, e)
    s = np.ldexp(1.0, e)
    inv_s = np.where(flush, 0.0, np.ldexp(1.0, -e))
    B = sum(np.ldexp(1.0, -1 - 7 * t) for t in range(KD))
    C = np.ldexp(1.0, 52 - 7 * KD) + B              # exact: B's last bit is 2^(6 - 7 KD), C's ulp is 2^(-7 KD)
    vv = np.where(bad[:, None, None], 0.0, v)
    # fma(v, 1/s, C): v / s is exact (a power of two, |v / s| < 1/2), so the product-then-sum rounds once, as the fma does
    y = vv * inv_s[:, None, None]
    z = y + C
    if perturb == "truncate":                       # round toward minus infinity instead of to nearest even
        back = y - (z - C)                          # exact: the rounding error of the sum
        z = np.where(back < 0.0, np.nextafter(z, 0.0), z)
    bits = z.view(np.uint64)
    dig = np.empty((2, KD, N, N), dtype=np.int64)
    for t in range(KD):
        byte = (bits >> np.uint64(7 * (KD - 1 - t))) & np.uint64(127)      # the offset byte d_t + 64
        dig[0, t] = byte[:, :, 0].astype(np.int64) - 64
        dig[1, t] = byte[:, :, 1].astype(np.int64) - 64
    sums = np.cumsum(dig.sum(axis=3), axis=1)       # [2][KD][N]
    s = np.where(bad, np.nan, s)
    return {"s": s, "dr": dig[0], "di": dig[1], "sums": sums}


def _gemm_int(P, Q):
    """P @ Q^T for integer-valued float64 matrices: every sum stays below 2^31 (asserted), so every partial sum is an
    exact double in any order."""
    G = P @ Q.T
    assert np.all(np.abs(G) < 2.0 ** 31), "an int32 accumulator group would overflow"
    return G.astype(np.int64)


def groups(sa, sm, KD, perturb=None):
    """The three times KD int32 accumulator groups of one product after the offset correction:
       G[tau][s][i][j], tau = 0, 1, 2 for U1 = ar.mr, U2 = ai.mi, U3 = (ar + ai).(mi - mr); s = a + b.
       (The pairs of one group are summed by ONE float64 GEMM over the concatenated k ranges: (s + 1) N terms, still exact.)"""
    N = sa["dr"].shape[1]
    G = np.zeros((3, KD, N, N), dtype=np.int64)
    f = np.float64
    left = ((sa["dr"] + 64).astype(f), (sa["di"] + 64).astype(f),       # multiplied on the offset bytes x = d + 64 in [0, 127]
            (sa["dr"] + sa["di"]).astype(f))                            # off_add: the int8 digits of (dr + di), in [-128, 126]
    right = ((sm["dr"] + 64).astype(f), (sm["di"] + 64).astype(f),
             (sm["di"] - sm["dr"]).astype(f))                           # off_sub: the int8 digits of (di - dr), in [-127, 127]
    for s in range(KD):
        pairs = [(a, s - a) for a in range(s + 1) if not (perturb == "drop_pair" and (a, s - a) == (0, KD - 1))]
        for tau in range(3):
            P = np.concatenate([left[tau][a] for a, _ in pairs], axis=1)
            Q = np.concatenate([right[tau][b] for _, b in pairs], axis=1)
            G[tau, s] = _gemm_int(P, Q)
    assert np.all(np.abs(G) < 2 ** 31)
    for tau in range(2):
        for s in range(KD):
            corr = 64 * sa["sums"][tau][s][:, None] + 64 * sm["sums"][tau][s][None, :] + 4096 * N * (s + 1)
            if perturb == "drop_pair" and s == KD - 1:      # the dropped pair's share of the offsets goes with it
                corr = corr - (64 * sa["sums"][tau][0][:, None] + 64 * (sm["sums"][tau][KD - 1] - (sm["sums"][tau][KD - 2] if KD > 1 else 0))[None, :]
                               + 4096 * N)
            if perturb == "correction" and s == KD - 1 and tau == 0:
                corr = corr + 64
            G[tau, s] -= corr
    return G


def convert(G, sa_s, sm_s, KD, perturb=None):
    """OZ_RESULT: t = sum over s from KD - 1 down to 0 of (double) g_s 2^(-7 (s + 2)) (small terms first; each product is
    exact, so the compiler's fma changes nothing), T = t (sa sb), Re = -(T0 + T1), Im = (T2 + T0) - T1.
    Returns (C, U) with U[tau] = T[tau]."""
    sc = sa_s[:, None] * sm_s[None, :]
    T = []
    for tau in range(3):
        t = np.zeros(G.shape[2:], dtype=np.float64)
        for s in range(KD - 1, -1, -1):
            w = np.ldexp(1.0, -7 * (s + 2))
            if perturb == "weight" and s == KD - 1:
                w = w * 128.0
            t = t + G[tau, s].astype(np.float64) * w
        T.append(t * sc)
    C = np.empty(G.shape[2:], dtype=np.complex128)
    C.real = -(T[0] + T[1])
    C.imag = (T[2] + T[0]) - T[1]
    return C, np.stack(T)


def leading(sl, KD):
    """The leading KD digits of a slicing with more: what k_oz_gemm<KD, ., KDM> gathers from M's planes and record."""
    return {"s": sl["s"], "dr": sl["dr"][:KD], "di": sl["di"][:KD], "sums": sl["sums"][:, :KD]}


def product(A, M, KD, KDM=None, perturb=None, details=False):
    """C = A @ B with B[k][j] = -conj(M[j][k]) as k_oz_slice<KD> (A), k_oz_slice<KDM> (M, by rows) and
    k_oz_gemm<KD, ., KDM> compute it.  KDM = 6 with KD = 5 multiplies the leading five digits of a six-digit slicing
    of M (QUFLOW_HIP_GEMM=i8x65's second product)."""
    KDM = KD if KDM is None else KDM
    sa = slice_rows(A, KD, perturb=perturb if perturb == "truncate" else None)
    sm = leading(slice_rows(M, KDM, perturb=perturb if perturb == "truncate" else None), KD)
    G = groups(sa, sm, KD, perturb=perturb)
    C, U = convert(G, sa["s"], sm["s"], KD, perturb=perturb)
    if details:
        return C, {"sa": sa, "sm": sm, "G": G, "U": U}
    return C


def constant_rows_product(drow, dcol_im, sa, sb, N, KD):
    """The product in closed form for A with rows constant along k and M = i c ones (skew-Hermitian), both given by
    their digits: A[i][k] = sa[i] sum_t (drow[0][t][i] + i drow[1][t][i]) 128^-(t+1), M[j][k] = i sb sum_t dcol_im[t] 128^-(t+1).
    Every group is N sum_{a + b = s} d_a e_b: no GEMM.  Returns (c, G): the column c[i] every C[i][j] equals, and the
    groups G[tau][s][i]."""
    n = drow.shape[2]
    G = np.zeros((3, KD, n, 1), dtype=np.int64)
    for a in range(KD):
        for b in range(KD - a):
            # U1 = ar.mr = 0 (mr = 0), U2 = ai.mi, U3 = (ar + ai).(mi - mr)
            G[1, a + b, :, 0] += N * drow[1][a] * int(dcol_im[b])
            G[2, a + b, :, 0] += N * (drow[0][a] + drow[1][a]) * int(dcol_im[b])
    assert np.all(np.abs(G) < 2 ** 31)
    assert 127 * 127 * N * KD < 2 ** 31              # the offset-form groups the kernel accumulates before the correction
    return convert(G, sa, np.full(1, sb), KD)[0][:, 0], G[:, :, :, 0]


def value_of_digits(d, s):
    """s sum_t d_t 128^-(t+1) for digits d [KD, ...] and scales s broadcast over the trailing axes: exact in a double
    for KD <= 7 (an integer below 2^50 times a power of two)."""
    KD = d.shape[0]
    n = np.zeros(d.shape[1:], dtype=np.int64)
    for t in range(KD):
        n = n * 128 + d[t]
    return n.astype(np.float64) * np.ldexp(1.0, -7 * KD) * s


def mirror_T(T, tile=TILE):
    """What the fused second product keeps of T = PW @ Phalf: the tiles above the diagonal tiles as computed, the ones
    below from -conj of their partner's, inside a diagonal tile the entries below the diagonal from above it -- i.e. the
    strict upper triangle as computed, the strict lower one its -conj transpose -- and Re T_ii = 0."""
    N = T.shape[0]
    up = np.triu(np.ones((N, N), dtype=bool), 1)
    out = np.zeros_like(T)
    out[up] = T[up]
    low = np.empty_like(T)
    low.real = -T.real.T                            # tre = -tp.x
    low.imag = T.imag.T                             # tim = tp.y
    out[up.T] = low[up.T]
    idx = np.arange(N)
    out[idx, idx] = 1j * T.imag[idx, idx]           # (+0.0 real part: the kernel stores the constant 0.0)
    return out


def fused_epilogue(T_upper, PW, W, dW_old, tile=TILE):
    """Everything FUSEDEPI writes, from the product's T (its entries on and above the diagonal are read), PW, the
    current W and the previous increment.  Additions only (2 comm is exact): nothing to contract.
    Returns dict(T, comm, dW, Whalf, W_next, Whalf_step, rowsum); rowsum[i] = sum_j |dW_old - dW|_ij in plain float64
    (the kernel sums its moduli in another order and may form them with an fma)."""
    T = mirror_T(T_upper, tile)
    comm = np.empty_like(PW)
    comm.real = PW.real - PW.real.T                 # cr = pw.x - pwt.x
    comm.imag = PW.imag + PW.imag.T                 # ci = pw.y + pwt.y
    dW = np.empty_like(PW)
    dW.real = T.real + comm.real
    dW.imag = T.imag + comm.imag
    Whalf = np.empty_like(PW)
    Whalf.real = W.real + dW.real
    Whalf.imag = W.imag + dW.imag
    W_next = np.empty_like(PW)
    W_next.real = W.real + 2.0 * comm.real
    W_next.imag = W.imag + 2.0 * comm.imag
    Wh_step = np.empty_like(PW)
    Wh_step.real = W_next.real + dW.real
    Wh_step.imag = W_next.imag + dW.imag
    rowsum = residual_row_sums(dW_old, dW)
    return {"T": T, "comm": comm, "dW": dW, "Whalf": Whalf, "W_next": W_next, "Whalf_step": Wh_step, "rowsum": rowsum}


def residual_row_sums(dW_old, dW):
    """sum_j |dW_old - dW|_ij with the moduli and the sums in np.longdouble (the differences are the kernel's own)."""
    er = (dW_old.real - dW.real).astype(np.longdouble)
    ei = (dW_old.imag - dW.imag).astype(np.longdouble)
    return np.sqrt(er * er + ei * ei).sum(axis=1).astype(np.float64)


def fp64_diagonal(A, M):
    """(value, bound) of the pair launch's fp64 diag[i] = sum_k (Re A_ik Im M_ik - Im A_ik Re M_ik) in np.longdouble,
    with sum_k |terms| for the tolerance."""
    ar, ai = A.real.astype(np.longdouble), A.imag.astype(np.longdouble)
    mr, mi = M.real.astype(np.longdouble), M.imag.astype(np.longdouble)
    val = (ar * mi - ai * mr).sum(axis=1)
    mag = (np.abs(ar * mi) + np.abs(ai * mr)).sum(axis=1)
    return val.astype(np.float64), mag.astype(np.float64)


def old_bound_holds(C, A, B, digits):
    """tests/test_hip_parity.py::test_zgemm_i8_vs_numpy's two criteria, restated for the sensitivity demonstration."""
    N = A.shape[0]
    ref = A @ B
    rowscale = np.abs(A).max(axis=1, keepdims=True)
    colscale = np.abs(B).max(axis=0, keepdims=True)
    ulp = 2.0 ** (-7 * digits)
    ok1 = np.all(np.abs(C - ref) <= 16 * N * ulp * rowscale * colscale)
    ok2 = np.all(np.abs(C - ref) <= 4 * np.sqrt(N) * ulp * 4 * rowscale * colscale)
    return bool(ok1 and ok2)


# ---- operands the host and the GPU tests share
def graded_operands(N, seed):
    """The operands of tests/test_hip_parity.py::test_zgemm_i8_vs_numpy: general A with rows spanning eight orders of
    magnitude times a skew-Hermitian M that decays off the diagonal."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    A *= (10.0 ** rng.uniform(-6, 2, size=(N, 1)))
    A[0, 1] += 7.0
    B = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    B = B - B.conj().T
    B *= np.exp(-0.05 * np.abs(np.subtract.outer(np.arange(N), np.arange(N))))
    return A, np.ascontiguousarray(B)


def on_grid(N, KD, seed, skew=False, spread=8):
    """A matrix whose entries ARE KD-digit values of their row's scale (slicing it is exact); the rows' scales are
    2^e, e drawn from [-spread, spread] (skew: skew-Hermitian, one scale)."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-64, 64, size=(2, KD, N, N))
    d[:, 0] = rng.integers(-62, 63, size=(2, N, N))
    e = rng.integers(-spread, spread + 1, size=N)
    X = value_of_digits(d[0], 1.0) + 1j * value_of_digits(d[1], 1.0)
    if skew:
        e[:] = 0
        X = np.triu(X, 1)
        X = X - X.conj().T + 1j * np.diag(value_of_digits(d[1], 1.0).diagonal())
    return np.ascontiguousarray(X * np.ldexp(1.0, e)[:, None])


def constant_rows_case(N, KD):
    """A with rows constant along k, built from crafted digit patterns (the extremes -64 and 63 included), M = i c ones:
    returns (drow [2][KD][N], e [KD], a [N] the rows' values, m the value of every entry of M, sb M's scale)."""
    pats = [[63] + [0] * (KD - 1), [-62] + [-64] * (KD - 1), [62] + [63] * (KD - 1), [63] + [-64] * (KD - 1), [-63] + [63] * (KD - 1),
            [1] + [-64, 63] * 3, [0] * (KD - 1) + [1], [0] * KD]
    rng = np.random.default_rng(0)
    drow = np.zeros((2, KD, N), dtype=np.int64)
    for i in range(N):
        drow[0, :, i] = pats[i % len(pats)][:KD]
        drow[1, :, i] = pats[(i // len(pats)) % len(pats)][:KD]
        if i >= len(pats) ** 2:
            drow[:, :, i] = rng.integers(-64, 64, size=(2, KD))
            drow[:, 0, i] = rng.integers(-62, 63, size=2)
        if max(abs(drow[0, 0, i]), abs(drow[1, 0, i])) < 33:        # keep the row's scale where the digits were built for
            drow[0, 0, i] = 62
    e = np.array([62] + [63] * (KD - 1))               # same sign throughout: nothing cancels in a group
    sa = np.ldexp(1.0, (np.arange(N) % 5) - 2)
    sb = 4.0
    a = value_of_digits(drow[0], sa) + 1j * value_of_digits(drow[1], sa)
    m = 1j * value_of_digits(e.reshape(KD, 1), sb)[0]
    return drow, e, a, m, sa, sb
