"""The int8 digit-split products (csrc/ozaki.hip) held digit for digit to tests/i8_mirror.py, a numpy restatement of their
arithmetic that tests/test_i8_mirror_host.py checks on the CPU: exact integer sums followed by a fixed sequence of IEEE
operations, so the assertion is equality of BITS, not a truncation-sized bound.

  * the plain product (qf_zgemm_i8: k_oz_slice<5|6> in its two-operand form, k_oz_gemm<5|6, plain>) at one tile, 2 x 2 tiles,
    an odd tile count and the production size, on graded, white and smooth data, on every edge of the slicing rule, and with
    the largest accumulator groups at N = 4096;
  * the fused kernels (k_oz_gemm<5|6, fused>, <5, fused, 6>), one iteration per step through qf_isomp(minit = maxit = 1) and the
    device's own Phalf / PW / dW / W / Whalf (qf_download_buffer), one and two steps;
  * what a non-finite entry does under the int8 modes.

No case needed the 2-ulp fallback: every comparison of the int8 kernels' output below is bit for bit.  What is NOT bit for bit,
by construction: Im PW_ii (fp64 row products of the slicing launch, another summation order), the residual norm (row sums of
moduli in the kernel's order) and the fp64 second product of i8x6f.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import i8_mirror as mir

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
MODES = {   # QUFLOW_HIP_GEMM -> (digits of the first product or None for fp64, (KD, KDM) of the second or None for fp64)
    "i8": (5, (5, 5)),
    "i8x6": (6, (6, 6)),
    "i8x65": (6, (5, 6)),
    "i8h": (None, (5, 5)),
    "i8x6f": (6, None),
}


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


@contextlib.contextmanager
def products(mode):
    """QUFLOW_HIP_GEMM / QUFLOW_HIP_I8_MIN_N for the contexts created inside (they are read when a context is created)."""
    old = {k: os.environ.get(k) for k in ("QUFLOW_HIP_GEMM", "QUFLOW_HIP_I8_MIN_N")}
    os.environ["QUFLOW_HIP_GEMM"] = mode
    os.environ["QUFLOW_HIP_I8_MIN_N"] = "64"
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bits(a):
    """The two IEEE words of every entry: shape + (2,)."""
    a = np.ascontiguousarray(a, dtype=np.complex128)
    return a.view(np.uint64).reshape(a.shape + (2,))


def zgemm_i8(A, M, digits):
    from quflow_amd import _lib
    from quflow_amd.context import Context, ptr
    A = np.ascontiguousarray(A, dtype=np.complex128)
    M = np.ascontiguousarray(M, dtype=np.complex128)
    C = np.full_like(A, np.nan)
    with products("i8" if digits == 5 else "i8x6"):
        ctx = Context(A.shape[0])
    try:
        _lib.check(ctx._lib.qf_zgemm_i8(ctx.handle, ptr(A), ptr(M), ptr(C)))
    finally:
        ctx.close()
    return C


def assert_product_bits(A, M, digits):
    C = zgemm_i8(A, M, digits)
    ref = mir.product(A, M, digits)
    np.testing.assert_array_equal(bits(C), bits(ref))
    return C


# ----------------------------------------------------------------------------- the plain product: tile counts and data
def smooth_state(oracle, N, seed):
    """solve_poisson(make_W0) renormalised: the rows' scales differ most (a few large low modes, a long small tail)."""
    P = oracle.solve_poisson(oracle.make_W0(N, seed)).copy()
    return np.ascontiguousarray(P / np.abs(P).max())


@pytest.mark.parametrize("digits", [5, 6])
@pytest.mark.parametrize("N", [64, 128, 192, 1024])
def test_plain_product_bit_for_bit(qfa, oracle, N, digits):
    """64: one tile; 128: 2 x 2; 192: an odd tile count; 1024: the production size (tiles % 16 == 0: the XCD-aware tile
    order).  Graded rows (test_zgemm_i8_vs_numpy's data), white unit-norm states, smooth states."""
    A, M = mir.graded_operands(N, N)
    assert_product_bits(A, M, digits)
    W = oracle.make_W0(N, 1)
    S = smooth_state(oracle, N, 2)
    assert_product_bits(S, W, digits)            # the stepper's first product: Phalf @ Whalf
    if N <= 192:
        assert_product_bits(W, S, digits)


# ----------------------------------------------------------------------------- the plain product: edges of the slicing rule
def edge_operands(N, KD):
    """A on the digit grid with one special row per edge of k_oz_slice's rule; M skew-Hermitian on the grid."""
    A = mir.on_grid(N, KD, 31)
    M = mir.on_grid(N, KD, 32, skew=True)
    g = 128.0 ** -KD
    rng = np.random.default_rng(33)
    small = (rng.integers(-2 ** 20, 2 ** 20, size=(16, N)) + 1j * rng.integers(-2 ** 20, 2 ** 20, size=(16, N))) * 2.0 ** -24
    b = 63.0 / 64.0
    A[0] = 0.0                                                   # a zero row
    A[1] = small[1]; A[1, 5] = np.ldexp(b, 3)                    # row maximum exactly 63/64 2^e: s = 2^(e+1)
    A[2] = small[2]; A[2, 5] = np.nextafter(np.ldexp(b, 3), 99.0)   # one ulp above: s = 2^(e+2)
    A[3] = small[3]; A[3, 5] = 8.0j                              # exactly 2^e (in the imaginary part)
    A[4] = small[4]; A[4, N - 1] = -np.ldexp(b, -2)              # the maximum attained by a negative entry: leading digit -63
    A[5] = small[5]; A[5, N - 1] = 1j * np.ldexp(b, -2)          # ... and by a positive one: +63
    lead = rng.integers(-62, 63, size=(2, N))

    def from_low(low):
        d = np.empty((2, KD, N), dtype=np.int64)
        d[:, 0] = lead
        d[:, 1:] = np.asarray(low)[None, :, None]
        return mir.value_of_digits(d[0], 1.0) + 1j * mir.value_of_digits(d[1], 1.0)
    A[6] = from_low([-64] * (KD - 1)); A[6, 0] = 63.0 / 128.0     # low digits all -64 (row scale pinned at 1)
    A[7] = from_low([63] * (KD - 1)); A[7, 0] = 63.0 / 128.0      # ... all 63
    A[8] = from_low(([-64, 63] * 3)[:KD - 1]); A[8, 0] = 63.0 / 128.0   # ... alternating
    mid = A[7].copy()                                            # (., 63, 63, ..) + half a grid step: the carry runs through every digit
    A[9].real = np.nextafter(mid.real + 0.5 * g, 1.0); A[9].imag = np.nextafter(mid.imag + 0.5 * g, -1.0); A[9, 0] = 63.0 / 128.0
    A[10].real = mid.real + 0.5 * g; A[10].imag = mid.imag - 0.5 * g; A[10, 0] = 63.0 / 128.0     # exact midpoints: ties to even
    A[11] = A[10] * 2.0 ** 40; A[12] = A[9] * 2.0 ** -40
    return np.ascontiguousarray(A), M


@pytest.mark.parametrize("digits", [5, 6])
@pytest.mark.parametrize("N", [64, 128])
def test_plain_product_slicing_edges(qfa, N, digits):
    """Operands built from chosen digits (exact on the grid), one row per edge: zero row, row maxima at, one ulp above and a
    power of two above the scale boundary f = 63/64, the maximum on a negative and on a positive entry (the digit set is not
    symmetric), low digits all -64 / all 63 / alternating, one ulp either side of a grid midpoint (the rounding carry runs
    through every digit) and exact midpoints (ties to even)."""
    A, M = edge_operands(N, digits)
    sl = mir.slice_rows(A, digits)
    np.testing.assert_array_equal(sl["s"][:6], [1.0, 16.0, 32.0, 32.0, 0.5, 0.5])      # the scale jumps where the rule says
    assert sl["dr"][0, 4, N - 1] == -63 and sl["di"][0, 5, N - 1] == 63
    assert sl["dr"][:, 6, 1:].min() == -64 and sl["dr"][:, 7, 1:].max() == 63
    assert_product_bits(A, M, digits)
    Z = np.zeros_like(A)
    assert_product_bits(Z, M, digits)             # a zero matrix A
    assert_product_bits(A, Z, digits)             # M = 0
    # swapped roles: the edge rows as rows of the skew-Hermitian right operand
    E = np.triu(A, 1)
    E = np.ascontiguousarray(E - E.conj().T)
    assert_product_bits(mir.on_grid(N, digits, 35), E, digits)


@pytest.mark.parametrize("digits", [5, 6])
@pytest.mark.parametrize("N", [64, 128])
def test_plain_product_scales_far_apart(qfa, N, digits):
    """Rows of A at 2^-900 against M at 2^+800 and the other way round: the scales' product and the exact result are
    representable although 1 / s and s are at opposite ends of the exponent range."""
    A = mir.on_grid(N, digits, 41)
    M = mir.on_grid(N, digits, 42, skew=True)
    A1 = A.copy()
    A1[::2] *= 2.0 ** -900
    C = assert_product_bits(A1, M * 2.0 ** 800, digits)
    assert np.isfinite(C).all() and np.abs(C[0]).max() > 0
    A2 = A.copy()
    A2[1::2] *= 2.0 ** 800
    C = assert_product_bits(A2, M * 2.0 ** -900, digits)
    assert np.isfinite(C).all() and np.abs(C[1]).max() > 0


@pytest.mark.parametrize("digits", [5, 6])
@pytest.mark.parametrize("N", [64, 128])
def test_plain_product_subnormal_row(qfa, N, digits):
    """A row whose largest entry is subnormal.  1 / s overflowed for such a row (ldexp(1.0, -e), e < -1023): the fma gave
    inf or NaN and ITS mantissa bits became the digits -- every digit -64, a row of C of size N s sb/4 where the exact one is below
    N 2^-1023 sb.  k_oz_slice now flushes a row whose scale would be below the smallest normal power of two to zero digits
    (DESIGN.md 3.6); the mirror restates the rule.  Expected: finite, bit for bit the mirror's, and within the flushed row's
    own size of the exact product: |C_ij - exact| <= 2 N 2^-1023 sb_j (two real products of at most N terms below 2^-1023 sb_j/2)."""
    A = mir.on_grid(N, digits, 51)
    M = mir.on_grid(N, digits, 52, skew=True)
    rng = np.random.default_rng(53)
    tiny = 2.0 ** -1074
    A[3] = (rng.integers(-2 ** 40, 2 ** 40, size=N) + 1j * rng.integers(-2 ** 40, 2 ** 40, size=N)) * tiny     # max below 2^-1033
    A[N - 1] = 0.0
    A[N - 1, 7] = tiny                                           # the smallest subnormal alone in its row
    A[5] = A[6] * 2.0 ** -900                                   # small but normal: sliced as any other row
    sl = mir.slice_rows(A, digits)
    assert sl["s"][3] == 1.0 and not sl["dr"][:, 3].any() and sl["s"][5] < 2.0 ** -890 and sl["dr"][:, 5].any()
    C = assert_product_bits(A, M, digits)
    assert np.isfinite(C).all()
    sb = mir.slice_rows(M, digits)["s"]
    for i in (3, N - 1):
        exact = (A[i].astype(np.clongdouble)[None, :] * (-M.conj()).astype(np.clongdouble)).sum(axis=1)
        err = np.maximum(np.abs((C[i].real - exact.real).astype(float)), np.abs((C[i].imag - exact.imag).astype(float)))
        assert np.all(err <= 2 * N * 2.0 ** -1023 * sb), (i, err.max())
    # the same rows in the right operand
    E = np.triu(A, 1)
    E = np.ascontiguousarray(E - E.conj().T)
    C = assert_product_bits(mir.on_grid(N, digits, 54), E, digits)
    assert np.isfinite(C).all()


@pytest.mark.parametrize("digits", [5, 6])
def test_plain_product_nonfinite_entry_poisons_its_row_or_column(qfa, digits):
    """What qf_zgemm_i8 yields for an inf or a NaN in an operand.  fmax dropped a NaN from the row maximum and an infinite
    maximum skipped the scale rule, so the entry's mantissa bits became finite digits: the product laundered inf and NaN into
    finite numbers.  k_oz_slice now gives a row with a non-finite entry the scale NaN: the whole row of C (entry
    in A) or column of C (entry in M's row j: column j of B) is NaN, as IEEE arithmetic would leave at least the entries the value
    reaches, and every other entry keeps its bits."""
    N = 128
    A0, M0 = mir.graded_operands(N, 77)
    for poison in (np.nan, np.inf, -np.inf):
        for where in ("A_re", "A_im", "M"):
            A, M = A0.copy(), M0.copy()
            if where == "A_re":
                A[70, 3] = poison + 1j
            elif where == "A_im":
                A[N - 1, N - 1] = 1.0 + 1j * poison
            else:
                M[65, 2] = poison
                M[2, 65] = -poison
            C = zgemm_i8(A, M, digits)
            ref = mir.product(A, M, digits)
            nan = np.isnan(ref.real) & np.isnan(ref.imag)
            want = np.zeros((N, N), dtype=bool)
            if where == "A_re":
                want[70] = True
            elif where == "A_im":
                want[N - 1] = True
            else:
                want[:, 65] = True
                want[:, 2] = True
            np.testing.assert_array_equal(nan, want)
            np.testing.assert_array_equal(np.isnan(C.real) & np.isnan(C.imag), want)
            np.testing.assert_array_equal(bits(C)[~want], bits(ref)[~want])


def test_plain_product_largest_accumulators_n4096(qfa):
    """N = 4096, six digits: A's rows are constant along k, each built from a crafted digit pattern with the extremes -64 and
    63 in it, M = i c ones (skew-Hermitian) with digits (62, 63, 63, ...): every accumulator group is N sum_{a+b=s} d_a e_b in
    closed form -- the largest sums the int32 groups see at the largest N the slicing takes -- and the exact answer is known
    without a GEMM."""
    N, KD = 4096, 6
    drow, e, a, m, sa, sb = mir.constant_rows_case(N, KD)
    c, G = mir.constant_rows_product(drow, e, sa, sb, N, KD)
    assert np.abs(G).max() > 2 ** 26                             # (N 6 64 64 = 2^28 is the most a group of this shape can hold)
    A = np.empty((N, N), dtype=np.complex128)
    A[:] = a[:, None]
    M = np.full((N, N), m)
    C = zgemm_i8(A, M, KD)
    del A, M
    np.testing.assert_array_equal(bits(C[:, 0]), bits(c))
    assert np.all(bits(C) == bits(C[:, :1]))                     # every column the same bits


# ----------------------------------------------------------------------------- the fused kernels, one iteration per step
_runs = {}


def run_steps(qfa, oracle, mode, N, steps):
    """`steps` steps of qf_isomp(minit = maxit = 1, tol = 0) on a context of its own under QUFLOW_HIP_GEMM=mode, then the
    device's buffers.  After the call (api_isomp.hip, fused_leave): QF_BUF_W is the buffer of the W pair the last step's
    W_next went to; QF_BUF_DW is dW[dw_parity], the buffer the last second product wrote; QF_BUF_WHALF is, the step having closed
    (wh_sel = 1), the PREPARED Whalf_step = W_next + dW the next step's first iteration would read (the plain Whalf = W + dW of
    the closed iteration stays in the other buffer of that pair and is not downloadable); Phalf and PW are the last
    iteration's.  Runs are deterministic (the ensemble tests require it), so the two-step test takes step 1 from the
    one-step run.  Cached: one run per (mode, N, steps) for the module."""
    key = (mode, N, steps)
    if key in _runs:
        return _runs[key]
    from quflow_amd import _lib
    from quflow_amd.context import Context, ptr
    W0 = oracle.make_W0(N, 5)
    dt = 0.25 * qfa.hbar(N)
    with products(mode):
        ctx = Context(N)
    out = {"W0": W0}
    try:
        _lib.check(ctx._lib.qf_upload_W(ctx.handle, ptr(W0)))
        st = _lib.IsompStats()
        _lib.check(ctx._lib.qf_isomp(ctx.handle, float(dt), int(steps), 0.0, 1, 1, 0, 0, ctypes.byref(st)))
        for name in ("W", "dW", "Whalf", "Phalf", "PW"):
            buf = np.full((N, N), np.nan, dtype=np.complex128)
            _lib.check(ctx._lib.qf_download_buffer(ctx.handle, _lib.BUFFER_IDS[name], ptr(buf)))
            out[name.upper()] = buf
        out["stats"] = (int(st.total_iterations), int(st.number_of_maxit), float(st.last_resnorm))
        out["plan"] = ctx.plan()
    finally:
        ctx.close()
    _runs[key] = out
    return out


def check_plan(plan, mode, N):
    first, second = MODES[mode]
    tiles = N // 64
    fp = plan["first_product"]["kernel"]
    sp = plan["second_product"]["kernel"]
    sl = plan["slicing"]
    if first is None:
        assert fp.startswith("k_zgemm"), fp
    else:
        assert fp == "k_oz_gemm<%d,plain,%d>" % (first, first), fp
        assert plan["first_product"]["tile_share"] == 1.0
    if second is None:
        assert sp.startswith("k_zgemm_tri"), sp
        assert sl["kernel"] == "k_oz_slice<6>" and sl["operands"] == 2 and sl["fp64_diagonal_of_the_product"] is True, sl
    else:
        assert sp == "k_oz_gemm<%d,fused,%d>" % second, sp
        # the tiles on and above the diagonal multiply, the others take their partner's result
        assert abs(plan["second_product"]["tile_share"] - (tiles * (tiles + 1) / 2 if tiles > 1 else 1) / (tiles * tiles)) < 1e-6
        # the last slicing launch of an iteration: PW alone (both products int8) or PW and Phalf together (i8h)
        assert sl["kernel"] == "k_oz_slice<%d>" % second[0] and sl["digits"] == second[0], sl
        assert sl["operands"] == (2 if first is None else 1) and sl["fp64_diagonal_of_the_product"] is False, sl


def check_step(mode, N, run, Whalf_in, W_in, dW_old, iterations):
    """One closed step of one iteration against the mirror: PW from the downloaded Phalf and the Whalf the iteration read, T from
    the downloaded PW and Phalf, then everything the fused epilogue stored."""
    first, second = MODES[mode]
    Phalf, PW = run["PHALF"], run["PW"]
    off = ~np.eye(N, dtype=bool)
    np.testing.assert_array_equal(Phalf[off], (-Phalf.conj().T)[off])
    idx = np.arange(N)
    if first is not None:
        ref = mir.product(Phalf, Whalf_in, first)
        got = PW.copy()
        # Im PW_ii: the fp64 row products of the pair slicing launch, stored over the digit sum's value
        dval, dmag = mir.fp64_diagonal(Phalf, Whalf_in)
        assert np.all(np.abs(PW.imag[idx, idx] - dval) <= 4 * N * EPS * dmag)
        got.imag[idx, idx] = ref.imag[idx, idx]
        np.testing.assert_array_equal(bits(got), bits(ref))
    else:
        fp64 = Phalf @ Whalf_in
        assert np.abs(PW - fp64).max() <= 16 * EPS * N * (np.abs(Phalf) @ np.abs(Whalf_in)).max()
    if second is not None:
        T = mir.product(PW, Phalf, second[0], second[1])
        epi = mir.fused_epilogue(T, PW, W_in, dW_old)
        np.testing.assert_array_equal(bits(run["DW"]), bits(epi["dW"]))
        np.testing.assert_array_equal(bits(run["W"]), bits(epi["W_next"]))
        np.testing.assert_array_equal(bits(run["WHALF"]), bits(epi["Whalf_step"]))
    else:
        # i8x6f: the fp64 upper-triangle kernel forms T; held to test_fixedpoint_products_full_vs_triangle's bound
        # (that kernel keeps its own T_ii: the reference is the plain T + comm of that test, not the int8 kernels' mirrored T)
        comm = PW - PW.conj().T
        bound = 16 * EPS * N * (np.abs(PW) @ np.abs(Phalf)).max() + 4 * EPS * np.abs(PW).max()
        # on and above the diagonal, where that kernel multiplies: below it dW is -conj of the entry above (asserted exactly
        # further down), while the lower triangle of numpy's T differs from that by the skew defect the six-digit PW gives it
        up = np.triu(np.ones((N, N), dtype=bool))
        assert np.abs(run["DW"] - (PW @ Phalf + comm))[up].max() <= bound
        np.testing.assert_array_equal(run["W"], W_in + 2.0 * comm)           # W + 2 (PW - PW^H): no product in it
        assert np.abs(run["WHALF"] - (run["W"] + run["DW"]))[up].max() <= 2 * EPS * np.abs(run["W"]).max()
    np.testing.assert_array_equal(run["W"], -run["W"].conj().T)
    np.testing.assert_array_equal(run["DW"][off], (-run["DW"].conj().T)[off])
    if second is not None:
        # (the int8 kernels store Re T_ii = 0; the fp64 triangle kernel of i8x6f keeps its own Re T_ii, of rounding size -- inside
        # the bound above -- and the next Whalf and Phalf carry it on their diagonals)
        assert not run["DW"].real.diagonal().any() and not Phalf.real.diagonal().any()
    total, n_maxit, resnorm = run["stats"]
    assert total == iterations and n_maxit == iterations
    # the residual norm: the largest row sum of |dW_old - dW|; the kernel sums its moduli (qf_modulus, contractible) in its own order
    rows = mir.residual_row_sums(dW_old, run["DW"])
    assert abs(resnorm - rows.max()) <= 4 * N * EPS * rows.max(), (resnorm, rows.max())


@pytest.mark.parametrize("N", [64, 128, 192, 1024])
@pytest.mark.parametrize("mode", list(MODES))
def test_fused_one_step(qfa, oracle, mode, N):
    """One step of one iteration (N = 64: a single diagonal tile, no mirrored tiles; 128, 192: mirrored tiles, even and odd tile
    counts; 1024: production).  Whalf = W0 and dW_old = 0 at a call's first iteration."""
    run = run_steps(qfa, oracle, mode, N, 1)
    check_plan(run["plan"], mode, N)
    check_step(mode, N, run, run["W0"], run["W0"], np.zeros((N, N), dtype=np.complex128), 1)


@pytest.mark.parametrize("N", [64, 128, 192, 1024])
@pytest.mark.parametrize("mode", list(MODES))
def test_fused_two_steps(qfa, oracle, mode, N):
    """The second step's first product reads the prepared Whalf_step through X_alt (wh_sel), its epilogue reads dW_old != 0 and
    the W pair has flipped: step 1's W, dW and prepared Whalf from the one-step run, step 2 predicted from the second Phalf."""
    one = run_steps(qfa, oracle, mode, N, 1)
    two = run_steps(qfa, oracle, mode, N, 2)
    check_step(mode, N, two, one["WHALF"], one["W"], one["DW"], 2)


# ----------------------------------------------------------------------------- non-finite input under the int8 modes
def poisoned(W0, poison, where):
    N = W0.shape[0]
    Wb = W0.copy()
    if where == "diagonal":
        Wb[7, 7] = complex(0.0, poison)
    elif where == "off":
        Wb[3, 5] = poison
        Wb[5, 3] = -poison
    else:
        Wb[N - 2, 4] = complex(0.0, poison)
        Wb[4, N - 2] = complex(0.0, poison)
    return Wb


@pytest.mark.parametrize("N", [128, 1024])
@pytest.mark.parametrize("mode", ["i8x6", "i8x65", "i8h", "i8x6f"])
def test_nonfinite_state_raises_under_the_int8_modes(qfa, oracle, mode, N):
    """W0 with one NaN or one inf (on the diagonal, off it, in the last tile row), as
    test_nonfinite_state_raises_as_the_reference_does runs under the fp64 products: the same ValueError, the resident state
    as uploaded (in value: the triangle products' exit mirrors W's lower triangle, which may flip the sign of a zero), the context
    usable afterwards to the bits of a fresh one.  Such a state does reach the int8 kernels: the skew check that admits a state to
    them takes its maximum with fmax, which drops the NaN that x + (-conj x) gives in ONE component of an entry, so these states
    count as skew-Hermitian and are sliced (seen in the context's plan when this test was written).  The call still fails: with
    the NaN scale of k_oz_slice the entry's row and column of PW are NaN, the commutator and the residual with them."""
    W0 = oracle.make_W0(N, 0)
    dt = 0.25 * qfa.hbar(N)
    with products(mode):
        tr = qfa.DeviceTrajectory(W0)
        fresh = qfa.DeviceTrajectory(W0)
    try:
        for poison in (np.nan, np.inf):
            for where in ("diagonal", "off", "last_tile_row"):
                Wb = poisoned(W0, poison, where)
                tr.upload(Wb)
                with pytest.raises(ValueError, match="infs or NaNs"):
                    tr.advance(dt, 2)
                np.testing.assert_array_equal(tr.download(), Wb)                 # the state of the last completed step: none ran
        tr.upload(W0)
        s1 = tr.advance(dt, 2)
        s2 = fresh.advance(dt, 2)
        assert tr.ctx.plan()["slicing"] is not None
        np.testing.assert_array_equal(bits(tr.download()), bits(fresh.download()))
        assert s1["total_iterations"] == s2["total_iterations"]
    finally:
        tr.ctx.close()
        fresh.ctx.close()


@pytest.mark.parametrize("N", [128, 1024])
@pytest.mark.parametrize("mode", ["i8x6", "i8x65", "i8h", "i8x6f"])
def test_nonfinite_operand_inside_an_int8_call(qfa, oracle, mode, N):
    """A finite, exactly skew-Hermitian state that IS sliced and whose products leave the finite range inside the call: |W| =
    1e200, so PW = Phalf @ Whalf overflows in the first iteration and the second product's operands carry inf / NaN (int8 first
    product: sa sb overflows; fp64 first product: the sums do).  The call fails as the fp64 path does -- the same error, W as the
    last completed step left it (none: the uploaded bits), the context usable afterwards."""
    W0 = oracle.make_W0(N, 0)
    Wbig = np.ascontiguousarray(W0 * 1e200)
    np.testing.assert_array_equal(Wbig, -Wbig.conj().T)
    dt = 0.25 * qfa.hbar(N)
    with products(mode):
        tr = qfa.DeviceTrajectory(Wbig)
        fresh = qfa.DeviceTrajectory(W0)
    try:
        with pytest.raises(ValueError, match="infs or NaNs"):
            tr.advance(dt, 3)
        assert tr.ctx.plan()["slicing"] is not None
        np.testing.assert_array_equal(bits(tr.download()), bits(Wbig))
        tr.upload(W0)
        tr.advance(dt, 2)
        fresh.advance(dt, 2)
        np.testing.assert_array_equal(bits(tr.download()), bits(fresh.download()))
    finally:
        tr.ctx.close()
        fresh.ctx.close()


@pytest.mark.parametrize("mode", ["i8x6", "i8x65", "i8h", "i8x6f"])
def test_nonfinite_residual_mid_call_under_the_int8_modes(qfa, oracle, mode):
    """test_nonfinite_residual_mid_call_keeps_the_last_completed_step (dt = 1e7 hbar, one unconverged iteration per step: the
    exponent of |W| triples every step) under each int8 mode at N = 128: the call is closed at the step whose residual stops
    being finite, the resident state is finite, exactly skew-Hermitian and the oracle's state after m >= 2 completed steps, and
    the context runs a clean state afterwards."""
    import warnings
    N = 128
    W0 = oracle.make_W0(N, 0)
    dt = 1e7 * qfa.hbar(N)
    states = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for m in range(1, 12):
            Wc = W0.copy()
            try:
                oracle.isomp(Wc, dt, steps=m, minit=1, maxit=1)
            except ValueError as e:
                assert "infs or NaNs" in str(e)
                break
            states.append(Wc)
    assert 2 <= len(states) <= 9 and np.isfinite(states[-1]).all()
    with products(mode):
        tr = qfa.DeviceTrajectory(W0)
        fresh = qfa.DeviceTrajectory(W0)
    try:
        with pytest.raises(ValueError, match="infs or NaNs"):
            tr.advance(dt, 12, minit=1, maxit=1)
        assert tr.ctx.plan()["slicing"] is not None
        Wg = tr.download()
        assert np.isfinite(Wg).all()
        np.testing.assert_array_equal(Wg, -Wg.conj().T)
        # (the digit series carries 2^-35 .. 2^-42 per product and the unconverged map triples relative differences every step:
        # the bound of the existing test for the int8 products)
        rel = [float(np.abs(Wg - Wm).max() / np.abs(Wm).max()) for Wm in states]
        m = int(np.argmin(rel)) + 1
        assert rel[m - 1] <= 1e-6 and m >= 2, rel
        tr.upload(W0)
        tr.advance(0.25 * qfa.hbar(N), 2)
        fresh.advance(0.25 * qfa.hbar(N), 2)
        np.testing.assert_array_equal(bits(tr.download()), bits(fresh.download()))
    finally:
        tr.ctx.close()
        fresh.ctx.close()
