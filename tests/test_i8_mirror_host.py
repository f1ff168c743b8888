"""tests/i8_mirror.py (the numpy restatement of csrc/ozaki.hip that tests/test_hip_i8_digits.py holds the kernels to, bit
for bit) checked on the CPU before anything is compared with it: the digits' range and accuracy, the product against an
exact integer product of the same operands, and a demonstration that the bit-for-bit criterion catches low-order errors
the truncation-sized bound of test_zgemm_i8_vs_numpy lets through."""
from fractions import Fraction

import numpy as np
import pytest

import i8_mirror as mir

EPS = np.finfo(float).eps


graded = mir.graded_operands
on_grid = mir.on_grid


@pytest.mark.parametrize("KD", [5, 6])
def test_digits_range_and_accuracy(KD):
    N = 96
    A, M = graded(N, 5)
    A[7] = 0.0                                                   # a zero row
    A[8] = np.ldexp(63.0 / 64.0, 3)                              # the scale boundary itself
    A[9] = np.nextafter(np.ldexp(63.0 / 64.0, 3), 100.0)         # one ulp above it
    A[10] = -np.ldexp(63.0 / 64.0, -5) + 0j
    for X in (A, M):
        sl = mir.slice_rows(X, KD)
        s = sl["s"]
        assert np.all(np.frexp(s)[0] == 0.5)                     # powers of two
        m = np.abs(X.view(float).reshape(N, -1)).max(axis=1)
        assert np.all(m / s <= 63.0 / 128.0)
        nz = m > 0
        assert np.all(2.0 * m[nz] / s[nz] > 63.0 / 128.0)        # ... and the smallest such
        for c, part in (("dr", X.real), ("di", X.imag)):
            d = sl[c]
            assert d.min() >= -64 and d.max() <= 63
            assert d[0].min() >= -63 and d[0].max() <= 63
            y = part / s[:, None]                                # exact
            back = mir.value_of_digits(d, 1.0)                   # exact (an integer below 2^50 times 2^(-7 KD))
            assert np.all(np.abs(y - back) <= 0.5 * 128.0 ** -KD)
        np.testing.assert_array_equal(sl["sums"][0], np.cumsum(sl["dr"].sum(axis=2), axis=0))
    assert mir.slice_rows(A, KD)["s"][8] == 16.0 and mir.slice_rows(A, KD)["s"][9] == 32.0


def test_scale_rule_edges():
    """The scale jumps where k_oz_slice's frexp rule says: f <= 63/64 takes 2^(e+1), above it 2^(e+2); a zero row and a
    row at or above 1e300 take 1; a row below the smallest normal scale is flushed; a non-finite entry gives a NaN scale."""
    N = 16
    X = np.zeros((N, N), dtype=complex)
    b = 63.0 / 64.0
    X[0, 3] = b
    X[1, 3] = np.nextafter(b, 2.0)
    X[2, 3] = 1.0
    X[3, 3] = -1j * b
    X[4, 3] = 5e-324
    X[5, 3] = 2.0 ** -1025                          # s would be 2^-1023: below the smallest normal power of two
    X[6, 3] = 2.0 ** -1022 * b                       # 1 / s = 2^1022: still representable, not flushed
    X[7, 3] = np.nan
    X[8, 3] = -1j * np.inf
    X[9, 3] = 1e300
    sl = mir.slice_rows(X, 5)
    np.testing.assert_array_equal(sl["s"][[0, 1, 2, 3, 4, 5, 6, 9, 10]],
                                  [2.0, 4.0, 4.0, 2.0, 1.0, 1.0, 2.0 ** -1021, 1.0, 1.0])
    assert np.isnan(sl["s"][7]) and np.isnan(sl["s"][8])
    assert not sl["dr"][:, 4].any() and not sl["dr"][:, 5].any() and sl["dr"][0, 6, 3] == 63
    assert sl["di"][0, 3, 3] == -63 and sl["dr"][0, 0, 3] == 63 and sl["dr"][0, 1, 3] == 32 and sl["dr"][0, 2, 3] == 32


def test_rounding_carries_and_ties():
    """Values one ulp on either side of a grid midpoint round apart, the carry running through every digit; an exact
    midpoint goes to the even grid point (the fma's tie rule)."""
    KD = 5
    N = 16
    X = np.zeros((N, N), dtype=complex)
    X[:, 0] = 63.0 / 128.0                           # fixes every row's scale at 1
    g = 128.0 ** -KD
    low = [63] * KD                                  # d = (0, 63, 63, 63, 63) + half a grid step carries into the leading digit
    low[0] = 0
    base = mir.value_of_digits(np.array(low).reshape(KD, 1), 1.0)[0]
    X[0, 1] = base + 0.5 * g                         # exact midpoint: n odd below -> rounds up to even (carry through all)
    X[1, 1] = np.nextafter(base + 0.5 * g, 0.0)      # just below: stays
    X[2, 1] = np.nextafter(base + 0.5 * g, 1.0)      # just above: carries
    X[3, 1] = base - 0.5 * g                         # exact midpoint below: n - 1 is even -> rounds down
    sl = mir.slice_rows(X, KD)
    assert np.all(sl["s"] == 1.0)
    n = [int(sum(int(sl["dr"][t, i, 1]) * 128 ** (KD - 1 - t) for t in range(KD))) for i in range(4)]
    nb = sum(low[t] * 128 ** (KD - 1 - t) for t in range(KD))
    assert nb % 2 == 1
    assert n == [nb + 1, nb, nb + 1, nb - 1], (n, nb)
    assert list(sl["dr"][:, 0, 1]) == [1, -64, -64, -64, -64]         # the carry went through every digit
    assert list(sl["dr"][:, 1, 1]) == low


def exact_groups(sa, sm, KD):
    """All KD x KD digit-pair products of one real product triple in int64 (exact): G[tau][a][b][i][j]."""
    N = sa["dr"].shape[1]
    G = np.zeros((3, KD, KD, N, N), dtype=np.int64)
    for a in range(KD):
        for b in range(KD):
            G[0, a, b] = sa["dr"][a] @ sm["dr"][b].T
            G[1, a, b] = sa["di"][a] @ sm["di"][b].T
            G[2, a, b] = (sa["dr"][a] + sa["di"][a]) @ (sm["di"][b] - sm["dr"][b]).T
    return G


@pytest.mark.parametrize("KD,KDM", [(5, 5), (6, 6), (5, 6)])
def test_product_against_exact_integers(KD, KDM):
    """Operands on the digit grid at N = 64: the exact product is a sum of integers.  The mirror equals the KEPT part of
    the series (pairs a + b < KD) to 4 ulp of |U1| + |U2| + |U3|, and the full product to the dropped part, which is
    computed exactly from the digits -- no multiple of a truncation estimate."""
    N = 64
    A = on_grid(N, KD, 3)
    M = on_grid(N, KDM, 4, skew=True)
    np.testing.assert_array_equal(M, -M.conj().T)
    C, det = mir.product(A, M, KD, KDM, details=True)
    sa, sm_full = mir.slice_rows(A, KD), mir.slice_rows(M, KDM)
    np.testing.assert_array_equal(mir.value_of_digits(sa["dr"], sa["s"][:, None]), A.real)      # slicing these is exact
    np.testing.assert_array_equal(mir.value_of_digits(sm_full["di"], sm_full["s"][:, None]), M.imag)
    G = exact_groups(sa, sm_full, max(KD, KDM)) if KD == KDM else None
    if G is None:                                    # 5 of 6: A has five digits, M six
        pad = {k: (np.concatenate([v, np.zeros_like(v[:1])]) if k in ("dr", "di") else v) for k, v in sa.items()}
        G = exact_groups(pad, sm_full, 6)
    K = G.shape[1]
    worst = 0.0
    for i in range(0, N, 7):
        for j in range(0, N, 5):
            sc = Fraction(float(sa["s"][i])) * Fraction(float(sm_full["s"][j]))
            kept, full = [], []
            for tau in range(3):
                k_ = sum(Fraction(int(G[tau, a, b, i, j]), 128 ** (a + b + 2)) for a in range(K) for b in range(K) if a + b < KD and a < KD and b < KD)
                f_ = sum(Fraction(int(G[tau, a, b, i, j]), 128 ** (a + b + 2)) for a in range(K) for b in range(K))
                kept.append(k_ * sc)
                full.append(f_ * sc)
            mag = float(sum(abs(x) for x in kept))
            re_k, im_k = -(kept[0] + kept[1]), kept[2] + kept[0] - kept[1]
            re_f, im_f = -(full[0] + full[1]), full[2] + full[0] - full[1]
            c = complex(C[i, j])
            assert abs(Fraction(c.real) - re_k) <= 4 * EPS * mag and abs(Fraction(c.imag) - im_k) <= 4 * EPS * mag
            dropped_re, dropped_im = abs(re_f - re_k), abs(im_f - im_k)
            assert abs(Fraction(c.real) - re_f) <= dropped_re + 4 * EPS * mag
            assert abs(Fraction(c.imag) - im_f) <= dropped_im + 4 * EPS * mag
            worst = max(worst, float(dropped_re / sc), float(dropped_im / sc))
            # the full integer product IS the product of the operands
            exact = sum(Fraction(float(A[i, k].real)) * Fraction(float(M[j, k].real)) for k in range(N))
            assert full[0] == exact
    assert 0.0 < worst < 3 * N * 2 ** 14 * 2 * K * 128.0 ** -(KD + 2)     # the dropped part is there, and of the size the series says
    # the mirror's own groups are the exact ones
    for s in range(KD):
        want = sum(G[:, a, s - a] for a in range(s + 1))
        np.testing.assert_array_equal(det["G"][:, s], want)


def test_kdm6_takes_the_leading_five_of_six_digits():
    A, M = graded(64, 9)
    six = mir.slice_rows(M, 6)
    five = mir.leading(six, 5)
    np.testing.assert_array_equal(five["dr"], six["dr"][:5])
    np.testing.assert_array_equal(five["sums"], six["sums"][:, :5])
    # the leading five of six are the value truncated, not rounded: they differ from a five-digit slicing somewhere
    assert np.any(five["dr"] != mir.slice_rows(M, 5)["dr"])
    assert np.any(mir.product(A, M, 5, 6).view(np.uint64) != mir.product(A, M, 5, 5).view(np.uint64))


@pytest.mark.parametrize("KD", [5, 6])
def test_sensitivity_bitwise_catches_what_the_old_bound_passes(KD):
    """Four low-order errors put into the mirror: each changes at least one entry's bits, so the bit-for-bit criterion of
    tests/test_hip_i8_digits.py rejects a kernel that made it; the bound of test_zgemm_i8_vs_numpy accepts at least the
    two smallest (an offset correction off by 64 in the last group, a digit truncated where it should be rounded)."""
    N = 128
    A, M = graded(N, N)
    good = mir.product(A, M, KD)
    assert mir.old_bound_holds(good, A, M, KD)
    passed_old = {}
    for p in ("drop_pair", "correction", "weight", "truncate"):
        bad = mir.product(A, M, KD, perturb=p)
        assert np.any(bad.view(np.uint64) != good.view(np.uint64)), p
        passed_old[p] = mir.old_bound_holds(bad, A, M, KD)
        print(p, "old bound holds:", passed_old[p], "max |diff| / (sa sb):",
              float(np.max(np.abs(bad - good) / (mir.slice_rows(A, KD)["s"][:, None] * mir.slice_rows(M, KD)["s"][None, :]))))
    assert passed_old["correction"] and passed_old["truncate"], passed_old


def test_fused_epilogue_structure():
    N = 128
    rng = np.random.default_rng(2)

    def skew():
        X = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        return X - X.conj().T

    T, PW, W, dWo = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N)), skew() + 0.1, skew(), skew()
    out = mir.fused_epilogue(T, PW, W, dWo)
    Tm = out["T"]
    np.testing.assert_array_equal(Tm, -Tm.conj().T)
    iu = np.triu_indices(N, 1)
    np.testing.assert_array_equal(Tm[iu], T[iu])
    np.testing.assert_array_equal(Tm.diagonal(), 1j * T.imag.diagonal())
    np.testing.assert_array_equal(out["comm"], PW - PW.conj().T)
    np.testing.assert_array_equal(out["dW"], Tm + out["comm"])
    np.testing.assert_array_equal(out["Whalf"], W + out["dW"])
    np.testing.assert_array_equal(out["W_next"], W + 2 * out["comm"])
    np.testing.assert_array_equal(out["Whalf_step"], out["W_next"] + out["dW"])
    np.testing.assert_allclose(out["rowsum"], np.abs(dWo - out["dW"]).sum(axis=1), rtol=8 * EPS * N)


def test_constant_rows_closed_form_matches_the_gemm_mirror():
    """The N = 4096 case of the GPU test in closed form, checked here against the GEMM mirror at N = 128."""
    N, KD = 128, 6
    drow, e, a, m, sa, sb = mir.constant_rows_case(N, KD)
    A = np.ascontiguousarray(np.repeat(a[:, None], N, axis=1))
    M = np.full((N, N), m)
    np.testing.assert_array_equal(M, -M.conj().T)
    C1 = mir.product(A, M, KD)
    sl = mir.slice_rows(A, KD)
    np.testing.assert_array_equal(sl["dr"][:, :, 0], drow[0])
    np.testing.assert_array_equal(sl["di"][:, :, 0], drow[1])
    np.testing.assert_array_equal(sl["s"], sa)
    assert mir.slice_rows(M, KD)["s"][0] == sb
    assert drow.min() == -64 and drow.max() == 63 and e.max() == 63
    c, G = mir.constant_rows_product(drow, e, sa, sb, N, KD)
    np.testing.assert_array_equal(C1.view(np.uint64), np.repeat(c[:, None], N, axis=1).view(np.uint64))
