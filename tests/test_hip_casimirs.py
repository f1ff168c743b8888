"""GPU tests of the Casimirs C_k = Re tr((iW)^k) / N, k <= 8 (qf_casimirs, qf_c64_casimirs, qf_states_casimirs,
qf_mhd_casimirs behind quflow_amd.casimirs and the trajectories' methods).

What is an equality and what is a bound:
  * on matrices whose entries have real and imaginary parts in {-1, 0, 1} every product and every partial sum is an integer
    below 2^53 in any order (the 3M product's intermediate sums included) as long as 4 tr(|W|^k) < 2^53, |W| the entrywise
    modulus rounded up to integers -- the test asserts that condition on the host and picks the density to meet it -- so the
    device value equals float(S_k) / N of numpy's (equally exact) float64 products BIT FOR BIT, through all four entry
    forms, the cross sums of the MHD form included;
  * a random skew-Hermitian W with norm_L2 = 1 against the same powers in long double (N <= 257) or numpy complex128
    (above): |dev - ref| <= 8 k N u |W|_F^k / N, u = 2^-53, the worst-case normwise bound of k - 1 chained products plus
    the sum -- a guard, not the instrument's resolution;
  * C_2, the magnetic C_2 and cross[0] against diagnostics(): the project's bar for a total against diagnostics(), 64 N eps
    of the sum of moduli (tests/test_hip_mhd_budget.py); a complex64 trajectory against the host form of its widened
    download: bit for bit;
  * a run that calls casimirs between two advances equals its twin that never did, np.array_equal, and two calls in a row
    return the same bits;
  * the refusals return their codes and leave the state readable.

Sizes: 33 (odd, one edge tile), 64, 100, 257, 768, 800 (32 x 32 product family, edge tiles above 768), 1024 (64 x 64 family;
528 tile pairs of the traces kernel, more than one block at every size above 33)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
U = 2.0 ** -53
SIZES = [33, 64, 100, 257, 768, 800, 1024]


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


_DATA = {}


def _cached(key, make):
    if key not in _DATA:
        a = make()
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def phase_real(k, z):
    """Re(i^k z), exactly."""
    return (z.real, -z.imag, -z.real, z.imag)[k % 4]


# ----------------------------------------------------------------------------- integer data
def int_matrix(N, seed, per_row=None, skew=False):
    """Real and imaginary parts in {-1, 0, 1}; per_row: at most that many nonzero entries in a row; skew: exactly
    skew-Hermitian (upper triangle drawn, diagonal imaginary)."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-1, 2, (N, N)) + 1j * rng.integers(-1, 2, (N, N))
    if per_row is not None:
        keep = np.zeros((N, N), dtype=bool)
        for i in range(N):
            keep[i, rng.choice(N, size=min(per_row, N), replace=False)] = True
        A = np.where(keep, A, 0)
    if skew:
        A = np.triu(A, 1)
        A = A - A.conj().T + 1j * np.diag(rng.integers(-1, 2, N))
        if per_row is not None:
            assert (A != 0).sum(axis=1).max() <= 2 * per_row
    return np.ascontiguousarray(A, dtype=np.complex128)


def powers(W, p):
    """[W, W^2, .., W^p] by the library's recipe: A_2 = W W, A_3 = A_2 W, A_4 = A_2 A_2."""
    A = [W]
    if p >= 2:
        A.append(W @ W)
    if p >= 3:
        A.append(A[1] @ W)
    if p >= 4:
        A.append(A[1] @ A[1])
    return A


def pair_sum(X, Y):
    """tr(X Y) = sum_ab X_ab Y_ba."""
    return (X * Y.T).sum()


def traces(W, kmax, V=None):
    """tr(W^k), k = 1..kmax, and with V: tr(V W^k), k = 1..ceil(kmax / 2)."""
    p = (kmax + 1) // 2
    A = powers(W, p)
    S = [np.trace(W)] + [pair_sum(A[k // 2 - 1], A[k - k // 2 - 1]) for k in range(2, kmax + 1)]
    X = [pair_sum(V, A[k - 1]) for k in range(1, p + 1)] if V is not None else None
    return S, X


def assert_exactness_condition(W, kmax, V=None):
    """4 tr(|W|^k) < 2^53 for k <= kmax (and 4 tr(|V| |W|^k) for the cross sums), |.| rounded up to integers."""
    M = np.ceil(np.abs(W))
    S, X = traces(M, kmax, None if V is None else np.ceil(np.abs(V)))
    for k, s in enumerate(S, 1):
        assert 4.0 * s.real < 2.0 ** 53, (W.shape[-1], k, s)
    for k, s in enumerate(X or [], 1):
        assert 4.0 * s.real < 2.0 ** 53, (W.shape[-1], "cross", k, s)


def exact_casimirs(W, kmax, V=None):
    N = W.shape[-1]
    assert_exactness_condition(W, kmax, V)
    S, X = traces(W, kmax, V)
    C = np.array([float(phase_real(k, s)) / N for k, s in enumerate(S, 1)])
    if V is None:
        return C
    return C, np.array([float(phase_real(k + 1, s)) / N for k, s in enumerate(X, 1)])


def integer_case(N, kind):
    """(W, Theta, kmax): dense for k <= 4 at every size, dense for k <= 8 at N = 33, at most 8 nonzeros per row for k <= 8
    above; `skew`: an exactly skew-Hermitian W (dense, k <= 4)."""
    def make():
        if kind == "dense4":
            return int_matrix(N, 10 + N), int_matrix(N, 20 + N), 4
        if kind == "skew4":
            return int_matrix(N, 30 + N, skew=True), int_matrix(N, 40 + N, skew=True), 4
        per_row = None if N == 33 else 8
        return int_matrix(N, 50 + N, per_row), int_matrix(N, 60 + N, per_row), 8
    return _cached(("int", N, kind), make)


@pytest.mark.parametrize("kind", ["dense4", "k8", "skew4"])
@pytest.mark.parametrize("N", SIZES)
def test_exact_on_integer_data(qfa, N, kind):
    W, Theta, kmax = integer_case(N, kind)
    ref_W = _cached(("exact", N, kind, "W"), lambda: exact_casimirs(W, kmax))
    ref_T, ref_X = _cached(("exact", N, kind, "pair"), lambda: exact_casimirs(Theta, kmax, W))
    assert np.any(ref_W[1:] != 0.0) and np.any(ref_X != 0.0)
    # host in
    got = qfa.casimirs(W, kmax)
    print("N=%d %s host in: %s" % (N, kind, got))
    assert got.shape == (kmax,) and np.array_equal(got, ref_W), (got, ref_W)
    # lower kmax: fewer stored powers, the same values
    for km in range(1, kmax):
        assert np.array_equal(qfa.casimirs(W, km), ref_W[:km]), km
    # resident
    tr = qfa.DeviceTrajectory(W)
    try:
        assert np.array_equal(tr.casimirs(kmax), ref_W)
    finally:
        tr.ctx.close()
    # stack members and the MHD pair
    st = qfa.DeviceMHDTrajectory(np.stack([W, Theta]))
    try:
        assert np.array_equal(st.casimirs(0, kmax), ref_W)
        assert np.array_equal(st.casimirs(1, kmax), ref_T)
        m = st.mhd_casimirs(kmax)
        print("N=%d %s cross: %s" % (N, kind, m["cross"]))
        assert m["magnetic"].shape == (kmax,) and m["cross"].shape == ((kmax + 1) // 2,)
        assert np.array_equal(m["magnetic"], ref_T), (m["magnetic"], ref_T)
        assert np.array_equal(m["cross"], ref_X), (m["cross"], ref_X)
        for km in range(1, kmax):
            mk = st.mhd_casimirs(km)
            assert np.array_equal(mk["magnetic"], ref_T[:km]) and np.array_equal(mk["cross"], ref_X[:(km + 1) // 2]), km
    finally:
        st.ctx.close()


# ----------------------------------------------------------------------------- random skew-Hermitian data
def random_skew(qfa, N, seed=0):
    return _cached(("W0", N, seed), lambda: qfa.ensemble.make_W0(N, seed))


def reference_casimirs(W, kmax=8):
    """N <= 257: the powers in long double; above: numpy complex128, as oracle.casimirs forms them (H = iW)."""
    N = W.shape[-1]
    if N <= 257:
        S, _ = traces(W.astype(np.clongdouble), kmax)
        return np.array([float(phase_real(k, s) / N) for k, s in enumerate(S, 1)])
    S, _ = traces(1j * W, kmax)
    return np.array([s.real / N for s in S])


@pytest.mark.parametrize("N", SIZES)
def test_random_skew_hermitian_against_reference(qfa, N):
    W = random_skew(qfa, N)
    assert abs(qfa.norm_L2(W) - 1.0) < 1e-14
    ref = _cached(("ref8", N), lambda: reference_casimirs(W))
    got = qfa.casimirs(W, 8)
    fro = np.linalg.norm(W, "fro")
    for k in range(1, 9):
        bar = 8 * k * N * U * fro ** k / N
        print("N=%d k=%d device %.17g reference %.17g diff %.3e bar %.3e" % (N, k, got[k - 1], ref[k - 1],
                                                                             abs(got[k - 1] - ref[k - 1]), bar))
        assert abs(got[k - 1] - ref[k - 1]) <= bar, k
    tr = qfa.DeviceTrajectory(W)
    try:
        assert np.array_equal(tr.casimirs(8), got)          # the resident form runs the same launches on the same data
    finally:
        tr.ctx.close()


# ----------------------------------------------------------------------------- against what the project already returns
def mhd_state(qfa, N):
    def make():
        W = qfa.ensemble.make_W0(N, 0)
        T = np.array(qfa.solve_poisson(qfa.ensemble.make_W0(N, 1)))
        T /= qfa.norm_L2(T)
        return np.stack([W, T])
    return _cached(("mhd", N), make)


@pytest.mark.parametrize("N", SIZES)
def test_second_casimir_is_twice_the_enstrophy(qfa, N):
    W = random_skew(qfa, N)
    tr = qfa.DeviceTrajectory(W)
    try:
        c = tr.casimirs()
        s = tr.diagnostics()[1]
    finally:
        tr.ctx.close()
    assert c.shape == (4,)
    print("N=%d C_2 %.17g 2 enstrophy %.17g" % (N, c[1], 2 * s))
    assert abs(c[1] - 2 * s) <= 64 * N * EPS * abs(2 * s)


@pytest.mark.parametrize("N", SIZES)
def test_mhd_members_against_diagnostics(qfa, N):
    state = mhd_state(qfa, N)
    st = qfa.DeviceMHDTrajectory(np.array(state))
    try:
        m = st.mhd_casimirs()
        d = st.diagnostics()
    finally:
        st.ctx.close()
    print("N=%d magnetic C_2 %.17g 2 A %.17g; cross[0] %.17g X %.17g" % (N, m["magnetic"][1], 2 * d["magnetic_casimir"],
                                                                      m["cross"][0], d["cross_helicity"]))
    assert abs(m["magnetic"][1] - 2 * d["magnetic_casimir"]) <= 64 * N * EPS * abs(2 * d["magnetic_casimir"])
    scale = (np.abs(state[0]) * np.abs(state[1])).sum() / N
    assert abs(m["cross"][0] - d["cross_helicity"]) <= 64 * N * EPS * scale


@pytest.mark.parametrize("N", [33, 100, 257, 1024])
def test_complex64_state_is_widened_exactly(qfa, N):
    W = random_skew(qfa, N).astype(np.complex64)
    tr = qfa.DeviceTrajectory(W)
    try:
        assert tr.c64
        got = tr.casimirs(8)
        back = tr.download()
    finally:
        tr.ctx.close()
    assert back.dtype == np.complex64 and np.array_equal(back, W)
    assert np.array_equal(got, qfa.physics.casimirs(back.astype(np.complex128), 8))
    assert np.array_equal(got, qfa.casimirs(back, 8))                   # complex64 host input goes through as_c128


def test_ensemble_member_by_member(qfa):
    N = 64
    ens = qfa.DeviceEnsemble([qfa.ensemble.make_W0(N, s) for s in range(3)])
    try:
        c = ens.casimirs(6)
        assert c.shape == (3, 6)
        for j, m in enumerate(ens.members):
            assert np.array_equal(c[j], m.casimirs(6))
            assert np.array_equal(c[j], qfa.casimirs(qfa.ensemble.make_W0(N, j), 6))
    finally:
        ens.close()


# ----------------------------------------------------------------------------- the run is untouched
@pytest.mark.parametrize("N,dtype", [(100, np.complex128), (1024, np.complex128), (100, np.complex64)])
def test_run_is_untouched(qfa, N, dtype):
    W0 = random_skew(qfa, N).astype(dtype)
    dt = 0.25 * qfa.hbar(N)
    a, b = qfa.DeviceTrajectory(W0), qfa.DeviceTrajectory(W0)
    try:
        sa, sb = a.advance(dt, 3), b.advance(dt, 3)
        assert sa == sb
        c1 = a.casimirs(8)
        c2 = a.casimirs(8)
        assert np.array_equal(c1, c2) and c1.tobytes() == c2.tobytes()
        sa, sb = a.advance(dt, 3, reinitialize=False), b.advance(dt, 3, reinitialize=False)
        assert sa == sb, (sa, sb)
        assert np.array_equal(a.download(), b.download())
        assert a.diagnostics() == b.diagnostics()
    finally:
        a.ctx.close()
        b.ctx.close()


def test_mhd_run_is_untouched(qfa):
    N = 100
    state = mhd_state(qfa, N)
    dt = 0.1 * qfa.hbar(N)
    a, b = qfa.DeviceMHDTrajectory(np.array(state)), qfa.DeviceMHDTrajectory(np.array(state))
    try:
        assert a.advance(dt, 3) == b.advance(dt, 3)
        m1, m2 = a.mhd_casimirs(8), a.mhd_casimirs(8)
        assert m1["magnetic"].tobytes() == m2["magnetic"].tobytes() and m1["cross"].tobytes() == m2["cross"].tobytes()
        assert a.casimirs(0, 8).tobytes() == a.casimirs(0, 8).tobytes()
        sa, sb = a.advance(dt, 3, reinitialize=False), b.advance(dt, 3, reinitialize=False)
        assert sa == sb, (sa, sb)
        assert np.array_equal(a.download(), b.download())
        assert a.diagnostics() == b.diagnostics()
    finally:
        a.ctx.close()
        b.ctx.close()


# ----------------------------------------------------------------------------- refusals
def test_refusals_leave_the_state_readable(qfa):
    from quflow_amd import _lib
    from quflow_amd.context import Context, ptr
    N = 33
    ctx = Context(N)
    lib = ctx._lib
    out = (ctypes.c_double * 8)()
    cross = (ctypes.c_double * 4)()
    try:
        # no resident state, no resident stack
        assert lib.qf_casimirs(ctx.handle, None, 4, out) == 4
        assert lib.qf_c64_casimirs(ctx.handle, 4, out) == 4
        assert lib.qf_states_casimirs(ctx.handle, 0, 4, out) == 4
        assert lib.qf_mhd_casimirs(ctx.handle, 4, out, cross) == 4
        W = np.ascontiguousarray(random_skew(qfa, N))
        _lib.check(lib.qf_upload_W(ctx.handle, ptr(W)))
        # bad arguments
        for kmax in (0, 9, -1):
            assert lib.qf_casimirs(ctx.handle, None, kmax, out) == 1
            assert lib.qf_casimirs(ctx.handle, ptr(W), kmax, out) == 1
        assert lib.qf_casimirs(ctx.handle, None, 4, None) == 1
        # a stack of three: no MHD form, members 0..2 only
        stack = np.ascontiguousarray(np.stack([W, 2 * W, 3 * W]))
        _lib.check(lib.qf_states_upload(ctx.handle, ptr(stack), 3))
        assert lib.qf_mhd_casimirs(ctx.handle, 4, out, cross) == 1
        assert lib.qf_states_casimirs(ctx.handle, 3, 4, out) == 1
        assert lib.qf_states_casimirs(ctx.handle, -1, 4, out) == 1
        assert lib.qf_states_casimirs(ctx.handle, 2, 4, out) == 0
        assert out[1] == qfa.casimirs(3 * W, 4)[1]
        back = np.empty_like(W)
        _lib.check(lib.qf_download_W(ctx.handle, ptr(back)))
        assert np.array_equal(back, W)
        sback = np.empty_like(stack)
        _lib.check(lib.qf_states_download(ctx.handle, ptr(sback), 3))
        assert np.array_equal(sback, stack)
        # a NaN entry: input data only
        bad = W.copy()
        bad[5, 7] = np.nan
        _lib.check(lib.qf_upload_W(ctx.handle, ptr(bad)))
        assert lib.qf_casimirs(ctx.handle, None, 4, out) == _lib.QF_ERR_NONFINITE
        assert lib.qf_casimirs(ctx.handle, ptr(bad), 8, out) == _lib.QF_ERR_NONFINITE
        _lib.check(lib.qf_download_W(ctx.handle, ptr(back)))
        assert np.array_equal(back, bad, equal_nan=True)
        with pytest.raises(ValueError, match="infs or NaNs"):
            qfa.casimirs(bad, 4)
        # and the context goes on working
        _lib.check(lib.qf_upload_W(ctx.handle, ptr(W)))
        assert lib.qf_casimirs(ctx.handle, None, 4, out) == 0
        assert np.array_equal(np.array(out[:4]), qfa.casimirs(W, 4))
    finally:
        ctx.close()
