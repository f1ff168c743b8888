"""What a `qf_ctx` carries between calls, against sequences of entry points that were written rounds apart, on the MI355X.

Between two calls a context keeps the resident state W, the iteration vector of the last qf_isomp call (`increment_valid`,
dW[dw_cur]: what qf_isomp_continue starts from), whether W is known to be exactly skew-Hermitian, and the scratch matrices
stage, Phalf, PW, Whalf, dW[0..1] that nearly every entry point stages through.  Every expectation here is another run of the
same library (byte for byte) or the CPU oracle; no figure comes from the code under test.

  A. READ_ONLY, the intervening-call matrix (raw ABI, one private context per size that is never released between the cases,
     so the entries also follow each other in every order the table gives).  For every entry E:
       * E's output equals its output on a fresh context that holds the same state,
       * qf_isomp(2); E; qf_isomp(2)           gives the state and statistics of the chain without E,
       * qf_isomp(1); E; qf_isomp_continue(1)  gives the state and statistics of the chain without E.
     The chains without E are run once per size on a context of their own; they move (the 2+2 state differs from the state
     after two steps) and the carried increment matters (qf_isomp(1); qf_isomp(1) gives other bytes or counts than
     qf_isomp(1); qf_isomp_continue(1)), so a dropped or a damaged increment shows.  A new entry point is one line of READ_ONLY.
  B. REPLACING: entries that replace the state or use dW[] as scratch end a carried increment: after qf_isomp(1); E a
     qf_isomp_continue(1) equals qf_isomp(1) on a fresh context that holds E's downloaded state -- state, iteration count,
     maxit count, tolerance.  After qf_erk with skewh = 0 the state is not exactly skew-Hermitian and the plan names the full
     second product.  The two ways a Strang half step reaches the state KEEP the increment (the reference's dW lives through
     strang_splitting, isospectral.py:466-482): qf_upload_W by contract, and the resident form of qf_solve_tridiagonal, which
     is "download, solve, upload" without the bus -- both are held to exactly that sequence.  complex64 (N = 100):
     qf_c64_solve_tridiagonal and qf_c64_upload_W both end the increment.
  C. Nested hooked steppers through the Python layer (N = 100, 768): a hook that itself runs hooked steppers at the same N
     neither disturbs the run it interrupts nor is disturbed by it, on the stepwise route (callback, strang_splitting) and
     inside qf_isomp_hooked (forcing); with the oracle's heun in the hook the oracle agrees within STEP_TOL = 1e-11 (the bar
     of test_hip_hooks_large.py) with identical iteration and maxit counts.

Sizes of A and B: 100 (guarded 32x32 tiles, deferred step end), 768 (32x32 triangle second product, folded solve), 1024
(64x64 first product, stream-K triangle, fused step end).  Data: oracle.make_W0(N, 0), dt = 0.25 hbar(N), tol 'auto'.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (100, 768, 1024)
NESTED_SIZES = (100, 768)
STEP_TOL = 1e-11
XI = (0.3, -0.2, 0.5)


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


# ----------------------------------------------------------------------------- raw ABI helpers
def _mods():
    from quflow_amd import _lib, context
    return _lib, context


def vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def call(ctx, name, *args):
    _lib, _ = _mods()
    _lib.check(getattr(ctx._lib, name)(ctx.handle, *args))


def upload(ctx, W, c64=False):
    Wc = np.ascontiguousarray(W)                   # (held until the call has returned)
    call(ctx, "qf_c64_upload_W" if c64 else "qf_upload_W", vp(Wc))


def download(ctx, c64=False):
    W = np.empty((ctx.N, ctx.N), dtype=np.complex64 if c64 else np.complex128)
    call(ctx, "qf_c64_download_W" if c64 else "qf_download_W", vp(W))
    return W


def isomp(ctx, dt, steps, cont=False, c64=False):
    """One qf_isomp / qf_isomp_continue call with the defaults of the Python layer; returns the statistics record's bytes."""
    _lib, _ = _mods()
    st = _lib.IsompStats()
    name = ("qf_c64_" if c64 else "qf_") + ("isomp_continue" if cont else "isomp")
    call(ctx, name, float(dt), int(steps), -1.0, 1, 10, 0, 0, ctypes.byref(st))
    return bytes(st)


def stats_of(raw):
    _lib, _ = _mods()
    st = _lib.IsompStats.from_buffer_copy(raw)
    return (st.total_iterations, st.number_of_maxit, st.tol_used, st.last_resnorm)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def skew(N, seed):
    from oracle import isomp_oracle
    W = isomp_oracle.make_W0(N, seed)
    W.setflags(write=False)
    return W


# ----------------------------------------------------------------------------- per size: inputs, the chains without E, the context
class Rig:
    def __init__(self, qfa, N):
        _lib, context = _mods()
        self.qfa, self.N = qfa, N
        self.dt = 0.25 * qfa.hbar(N)
        self.W0, self.X, self.X2, self.X3 = (skew(N, s) for s in range(4))
        rng = np.random.default_rng(100 + N)
        self.G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        self.G2 = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        self.Xc = self.X.astype(np.complex64)
        self.H = -1j * self.X                       # exactly Hermitian
        self.Ph, self.dW_old = 0.05 * self.X2, 0.01 * self.W0       # (skew-Hermitian operands of qf_fixedpoint_products)
        self.stack = np.ascontiguousarray(np.stack([self.X, self.X2]))
        self.tab, self.key = qfa.ViscDampStep(nu=1e-3, alpha=0.05).table_and_key(N, self.dt / 2)
        self.tab = np.ascontiguousarray(self.tab, dtype=np.float64)
        self.xi = np.array(XI, dtype=np.float64)
        self.omega = None                           # mat2shr(X): made with the basis
        # the chains without E, on a context of their own
        ref = context.Context(N)
        try:
            upload(ref, self.W0)
            self.s22 = (isomp(ref, self.dt, 2),)
            self.W2 = download(ref)
            self.s22 += (isomp(ref, self.dt, 2),)
            self.W4 = download(ref)
            upload(ref, self.W0)
            self.s11 = (isomp(ref, self.dt, 1),)
            self.W1 = download(ref)
            self.s11 += (isomp(ref, self.dt, 1, cont=True),)
            self.W11 = download(ref)
            upload(ref, self.W1)
            restart = isomp(ref, self.dt, 1)
            Wrestart = download(ref)
        finally:
            ref.close()
        print("N=%d chains: 2+2 %s %s   1+continue %s %s   1+restart %s" % (N, stats_of(self.s22[0]), stats_of(self.s22[1]),
              stats_of(self.s11[0]), stats_of(self.s11[1]), stats_of(restart)))
        assert not same(self.W4, self.W2) and not same(self.W2, self.W0), "the chain does not move"
        assert (self.W11.tobytes(), self.s11[1]) != (Wrestart.tobytes(), restart), "a dropped increment would not show"
        for a in (self.W1, self.W2, self.W4, self.W11):
            a.setflags(write=False)
        self.ctx = context.Context(N)               # the private context of every case of this size
        self.has_basis = False

    def need_basis(self):
        if not self.has_basis:
            call(self.ctx, "qf_basis_compute")
            self.omega = np.empty(self.N * self.N)
            call(self.ctx, "qf_mat2shr", vp(self.X), vp(self.omega), self.N * self.N)
            self.omega.setflags(write=False)
            self.has_basis = True

    def fresh(self, basis=False):
        _, context = _mods()
        c = context.Context(self.N)
        if basis:
            call(c, "qf_basis_compute")
        return c

    def close(self):
        self.ctx.close()


_RIGS = {}


@pytest.fixture(scope="module")
def rigs(qfa):
    def get(N):
        if N not in _RIGS:
            _RIGS[N] = Rig(qfa, N)
        return _RIGS[N]
    yield get
    for r in _RIGS.values():
        r.close()
    _RIGS.clear()


# ----------------------------------------------------------------------------- A. the read-only entries: fn(rig, ctx) -> outputs
def out(r, *shape, dtype=np.complex128):
    return np.empty(shape or (r.N, r.N), dtype=dtype)


def e_solve_poisson(r, c):
    P, Pg = out(r), out(r)
    call(c, "qf_solve_poisson", vp(r.X), vp(P), 1)
    call(c, "qf_solve_poisson", vp(r.G), vp(Pg), 0)
    return [P, Pg]


def e_laplace(r, c):
    Wl = out(r)
    call(c, "qf_laplace", vp(r.X), vp(Wl))
    return [Wl]


def e_solve_tridiagonal(r, c):
    P = out(r)
    call(c, "qf_solve_tridiagonal", vp(r.tab), ctypes.c_ulonglong(r.key), vp(r.X), vp(P), 1)
    return [P]


def e_hamiltonian(r, c):
    """P = T^-1 (W - F) of an installed table and offset; the built-in Hamiltonian is back before the next stepper call."""
    P = out(r)
    call(c, "qf_set_hamiltonian", vp(r.tab), ctypes.c_ulonglong(r.key), vp(r.X2), ctypes.c_ulonglong(22))
    try:
        call(c, "qf_hamiltonian", vp(r.X), vp(P))
    finally:
        call(c, "qf_clear_hamiltonian")
    return [P]


def e_hamiltonian_energy(r, c):
    H = ctypes.c_double(0.0)
    call(c, "qf_hamiltonian_energy", ctypes.byref(H))
    return [np.array([H.value])]


def e_forcing(r, c):
    F = out(r)
    call(c, "qf_set_forcing", vp(r.X2), ctypes.c_ulonglong(33), -0.05, 0.02, 1e-4)
    try:
        call(c, "qf_forcing", vp(r.X3), vp(r.X), vp(F))
    finally:
        call(c, "qf_clear_forcing")
    return [F]


def e_zgemm(r, c):
    C = out(r)
    call(c, "qf_zgemm", vp(r.G), vp(r.G2), vp(C))
    return [C]


def e_commutator(mode):
    def fn(r, c):
        C = out(r)
        call(c, "qf_commutator", vp(r.X), vp(r.X2), vp(C), mode)
        return [C]
    return fn


def e_products(triangle):
    def fn(r, c):
        variant = 0 if not triangle else (1 if r.N == 1024 else 2)      # the triangle form the stepper takes at this size
        dWn, Whn, rows = out(r), out(r), np.empty(r.N)
        call(c, "qf_fixedpoint_products", vp(r.Ph), vp(r.X), vp(r.X3), vp(r.dW_old), variant, vp(dWn), vp(Whn), vp(rows))
        return [dWn, Whn, rows]
    return fn


def e_diagnostics(r, c):
    e, z = ctypes.c_double(0.0), ctypes.c_double(0.0)
    call(c, "qf_diagnostics", ctypes.byref(e), ctypes.byref(z))
    return [np.array([e.value, z.value])]


def e_norm_inf(r, c):
    v = ctypes.c_double(0.0)
    call(c, "qf_norm_inf_W", ctypes.byref(v))
    return [np.array([v.value])]


def e_eigh(r, c):
    lam, V = np.empty(r.N), out(r)
    call(c, "qf_eigh", vp(r.H), vp(lam), vp(V), None)
    return [lam, V]


def e_eigh_state(r, c):
    lam = np.empty(r.N)
    call(c, "qf_eigh_state", vp(lam), None)
    return [lam]


def e_scale_decomposition(resident):
    def fn(r, c):
        Ws, Wr = out(r), out(r)
        call(c, "qf_scale_decomposition", None if resident else vp(r.X), None, vp(Ws), vp(Wr))
        return [Ws, Wr]
    return fn


def e_so3_exp(r, c):
    R = out(r)
    call(c, "qf_so3_exp", dp(r.xi), vp(R))
    return [R]


def e_rotate_host(r, c):
    R = out(r)
    call(c, "qf_rotate", dp(r.xi), vp(r.X), vp(R))
    return [R]


def e_grad(resident):
    def fn(r, c):
        dP = out(r, 3, r.N, r.N)
        call(c, "qf_grad", None if resident else vp(r.X), vp(dP))
        return [dP]
    return fn


def e_mat2shr_host(r, c):
    om = np.empty(r.N * r.N)
    call(c, "qf_mat2shr", vp(r.X), vp(om), r.N * r.N)
    return [om]


def e_shr2mat_host(r, c):
    Wm = out(r)
    call(c, "qf_shr2mat", vp(r.omega), r.N * r.N, vp(Wm))
    return [Wm]


def e_state_to_fun(r, c):
    """qf_mat2shr(NULL) leaves the state's coefficients on the device, qf_shr2fun(NULL) synthesises them."""
    L = min(r.N, 256)
    f = np.empty((L, 2 * L - 1))
    call(c, "qf_mat2shr", None, None, r.N * r.N)
    call(c, "qf_shr2fun", None, r.N * r.N, L, 1, vp(f))
    return [f]


def e_download_buffer(r, c):
    """Every buffer id is read; only W has contents a fresh context shares."""
    _lib, _ = _mods()
    got = {}
    for name, which in _lib.BUFFER_IDS.items():
        got[name] = out(r)
        call(c, "qf_download_buffer", which, vp(got[name]))
    return [got["W"]]


def e_c64_solve_poisson(r, c):
    P = out(r, dtype=np.complex64)
    call(c, "qf_c64_solve_poisson", vp(r.Xc), vp(P), 1)
    return [P]


# (id, entry, needs the quantization basis)
READ_ONLY = [
    ("solve_poisson", e_solve_poisson, False),
    ("laplace", e_laplace, False),
    ("solve_tridiagonal", e_solve_tridiagonal, False),
    ("hamiltonian", e_hamiltonian, False),
    ("hamiltonian_energy", e_hamiltonian_energy, False),
    ("forcing", e_forcing, False),
    ("zgemm", e_zgemm, False),
    ("commutator_skewherm", e_commutator(1), False),
    ("commutator_generic", e_commutator(0), False),
    ("fixedpoint_products_full", e_products(False), False),
    ("fixedpoint_products_triangle", e_products(True), False),
    ("diagnostics", e_diagnostics, False),
    ("norm_inf_W", e_norm_inf, False),
    ("eigh", e_eigh, False),
    ("eigh_state", e_eigh_state, False),
    ("scale_decomposition_host", e_scale_decomposition(False), False),
    ("scale_decomposition_state", e_scale_decomposition(True), False),
    ("so3_exp", e_so3_exp, False),
    ("rotate_host", e_rotate_host, False),
    ("grad_host", e_grad(False), False),
    ("grad_state", e_grad(True), False),
    ("mat2shr_host", e_mat2shr_host, True),
    ("shr2mat_host", e_shr2mat_host, True),
    ("mat2shr_state_shr2fun", e_state_to_fun, True),
    ("download_buffer", e_download_buffer, False),
    ("c64_solve_poisson", e_c64_solve_poisson, False),
]


@pytest.mark.parametrize("entry", READ_ONLY, ids=[e[0] for e in READ_ONLY])
@pytest.mark.parametrize("N", SIZES)
def test_intervening_call_leaves_the_trajectory_alone(rigs, N, entry):
    name, fn, basis = entry
    r = rigs(N)
    if basis:
        r.need_basis()
    c = r.ctx
    upload(c, r.W0)
    s = (isomp(c, r.dt, 2),)
    out2 = fn(r, c)
    s += (isomp(c, r.dt, 2),)
    W = download(c)
    assert s == r.s22 and same(W, r.W4), (name, N, "2 + E + 2", [stats_of(x) for x in s], [stats_of(x) for x in r.s22],
                                          float(np.abs(W - r.W4).max()))
    upload(c, r.W0)
    s = (isomp(c, r.dt, 1),)
    out1 = fn(r, c)
    s += (isomp(c, r.dt, 1, cont=True),)
    W = download(c)
    assert s == r.s11 and same(W, r.W11), (name, N, "1 + E + continue", [stats_of(x) for x in s], [stats_of(x) for x in r.s11],
                                           float(np.abs(W - r.W11).max()))
    for state, got in ((r.W2, out2), (r.W1, out1)):
        f = r.fresh(basis)
        try:
            upload(f, state)
            want = fn(r, f)
        finally:
            f.close()
        assert len(want) == len(got)
        for j, (a, b) in enumerate(zip(got, want)):
            assert np.all(np.isfinite(b)), (name, N, j)
            assert same(a, b), (name, N, "output %d differs from a fresh context's" % j, float(np.abs(a - b).max()))


# ----------------------------------------------------------------------------- B. entries that end a carried increment
def b_erk(method, skewh=1):
    def fn(r, c):
        call(c, "qf_erk", method, r.dt, 1, skewh)
    return fn


def b_isomp_simple(r, c):
    call(c, "qf_isomp_simple", r.dt, 1)


def b_isomp_quasinewton(r, c):
    _lib, _ = _mods()
    st = _lib.IsompStats()
    call(c, "qf_isomp_quasinewton", r.dt, 1, -1.0, 10, ctypes.byref(st))


def b_rotate_state(r, c):
    call(c, "qf_rotate", dp(r.xi), None, None)


def b_shr2mat_state(r, c):
    call(c, "qf_shr2mat", vp(r.omega), r.N * r.N, None)


def b_states_select(r, c):
    call(c, "qf_states_upload", vp(r.stack), 2)
    call(c, "qf_states_select", 1)


REPLACING = [
    ("erk_euler", b_erk(0), False),
    ("erk_heun", b_erk(1), False),
    ("erk_rk4", b_erk(2), False),
    ("erk_heun_general", b_erk(1, skewh=0), False),
    ("isomp_simple", b_isomp_simple, False),
    ("isomp_quasinewton", b_isomp_quasinewton, False),
    ("rotate_state", b_rotate_state, False),
    ("shr2mat_state", b_shr2mat_state, True),
    ("states_select", b_states_select, False),
]


@pytest.mark.parametrize("entry", REPLACING, ids=[e[0] for e in REPLACING])
@pytest.mark.parametrize("N", SIZES)
def test_replacing_call_ends_the_increment(rigs, N, entry):
    name, fn, basis = entry
    r = rigs(N)
    if basis:
        r.need_basis()
    c = r.ctx
    upload(c, r.W0)
    isomp(c, r.dt, 1)
    fn(r, c)
    WE = download(c)
    got = stats_of(isomp(c, r.dt, 1, cont=True))
    W = download(c)
    assert np.all(np.isfinite(WE)) and not same(WE, r.W1), (name, N, "E did not replace the state")
    f = r.fresh()
    try:
        upload(f, WE)
        want = stats_of(isomp(f, r.dt, 1))
        Wf = download(f)
    finally:
        f.close()
    print("%s N=%d: continue after E %s   fresh qf_isomp %s   max|dW| = %.3e" % (name, N, got, want, float(np.abs(W - Wf).max())))
    assert got[:3] == want[:3] and same(W, Wf), (name, N, got, want, float(np.abs(W - Wf).max()))
    if name == "erk_heun_general":
        assert not np.array_equal(WE, -WE.conj().T), "the general Runge-Kutta step left an exactly skew-Hermitian state"
        second = c.plan()["second_product"]
        assert second["kernel"].startswith("k_zgemm<") and second["tile_share"] == 1.0, second


@pytest.mark.parametrize("N", SIZES)
def test_strang_paths_keep_the_increment(rigs, N):
    """qf_upload_W keeps the increment by contract (quflow_hip.h, qf_isomp_continue): the round trip through the host changes
    nothing.  The resident form of qf_solve_tridiagonal is the same half step without the bus: it equals download, host-form
    solve, upload -- and so differs from a restart, which the chains of the rig already told apart."""
    r = rigs(N)
    c = r.ctx
    upload(c, r.W0)
    s = (isomp(c, r.dt, 1),)
    upload(c, download(c))
    s += (isomp(c, r.dt, 1, cont=True),)
    W = download(c)
    assert s == r.s11 and same(W, r.W11), (N, "round trip", [stats_of(x) for x in s], [stats_of(x) for x in r.s11])

    key = ctypes.c_ulonglong(r.key)
    upload(c, r.W0)
    isomp(c, r.dt, 1)
    call(c, "qf_solve_tridiagonal", vp(r.tab), key, None, None, 1)
    Wa_mid = download(c)
    sa = isomp(c, r.dt, 1, cont=True)
    Wa = download(c)

    upload(c, r.W0)
    isomp(c, r.dt, 1)
    Wb_one, Wb_mid = download(c), np.empty_like(Wa_mid)
    call(c, "qf_solve_tridiagonal", vp(r.tab), key, vp(Wb_one), vp(Wb_mid), 1)
    upload(c, Wb_mid)
    sb = isomp(c, r.dt, 1, cont=True)
    Wb = download(c)
    print("N=%d resident half step: %s   through the host: %s" % (N, stats_of(sa), stats_of(sb)))
    assert same(Wa_mid, Wb_mid) and not same(Wa_mid, r.W1)
    assert sa == sb and same(Wa, Wb), (N, stats_of(sa), stats_of(sb), float(np.abs(Wa - Wb).max()))


def test_complex64_upload_and_table_solve_end_the_increment(rigs):
    """complex64, N = 100: qf_c64_solve_tridiagonal builds its factors in dW[1] and qf_c64_upload_W starts afresh; after either
    a qf_c64_isomp_continue equals qf_c64_isomp on a fresh context with the same state.  (Existing behaviour, pinned.)"""
    N = 100
    r = rigs(N)
    c = r.ctx
    W0 = r.W0.astype(np.complex64)
    tab32 = np.ascontiguousarray(r.tab, dtype=np.float32)

    def solve(ctx):
        P = np.empty((N, N), dtype=np.complex64)
        call(ctx, "qf_c64_solve_tridiagonal", vp(tab32), vp(r.Xc), vp(P), 1)
        return P

    def round_trip(ctx):
        upload(ctx, download(ctx, c64=True), c64=True)

    f = r.fresh()
    try:
        P_fresh = solve(f)
    finally:
        f.close()
    for name, E in (("c64_solve_tridiagonal", solve), ("c64_upload_W", round_trip)):
        upload(c, W0, c64=True)
        first = stats_of(isomp(c, r.dt, 1, c64=True))
        res = E(c)
        WE = download(c, c64=True)
        got = stats_of(isomp(c, r.dt, 1, cont=True, c64=True))
        W = download(c, c64=True)
        f = r.fresh()
        try:
            upload(f, WE, c64=True)
            want = stats_of(isomp(f, r.dt, 1, c64=True))
            Wf = download(f, c64=True)
        finally:
            f.close()
        print("%s: first %s   continue after E %s   fresh %s" % (name, first, got, want))
        assert not same(WE, W0) and np.all(np.isfinite(W))
        assert got[:3] == want[:3] and same(W, Wf), (name, got, want)
        if res is not None:
            assert same(res, P_fresh)


# ----------------------------------------------------------------------------- C. nested hooked steppers, Python layer
def force(P, W):
    return -0.05 * W + 0.02 * P


def make_foreign(oracle):
    def foreign(W):
        return 0.5 * oracle.solve_poisson(W) + 0.1j * np.eye(W.shape[-1])
    return foreign


def noop(W, dW):
    pass


class Inner:
    """The three hooked stepper calls a hook makes on an unrelated fixed V of the same N, and what they return outside any
    hook (made once per size)."""

    def __init__(self, qfa, oracle, N):
        self.qfa, self.N = qfa, N
        self.dt = 0.25 * qfa.hbar(N)
        self.V = skew(N, 7)
        self.foreign = make_foreign(oracle)
        self.want = self.run()
        self.seen = []

    def run(self):
        qfa, V, dt = self.qfa, self.V, self.dt
        sa, sb = {"iterations": 0.0}, {}
        return (qfa.heun(V.copy(), dt / 2, 1, forcing=force),
                qfa.isomp(V.copy(), dt, 1, callback=noop, stats=sa), sa,
                qfa.isomp_quasinewton(V.copy(), dt, 1, hamiltonian=self.foreign, stats=sb), sb)

    def __call__(self):
        self.seen.append(self.run())

    def check(self, calls):
        assert len(self.seen) == calls, (len(self.seen), calls)
        for got in self.seen:
            for a, b in zip(got, self.want):
                assert (a == b) if isinstance(a, dict) else same(a, b), (self.N, "an inner result differs from the call outside a hook")
        self.seen = []


_INNER = {}


@pytest.fixture(scope="module")
def inner(qfa, oracle):
    def get(N):
        if N not in _INNER:
            _INNER[N] = Inner(qfa, oracle, N)
        return _INNER[N]
    return get


def run_isomp(qfa, W0, dt, steps, **kw):
    st = {"iterations": 0.0}
    W = qfa.isomp(W0.copy(), dt, steps, stats=st, **kw)
    return W, st


@pytest.mark.parametrize("route", ["callback", "strang_splitting", "forcing"])
@pytest.mark.parametrize("N", NESTED_SIZES)
def test_nested_hooked_steppers_do_not_interfere(qfa, inner, N, route):
    """callback / strang_splitting: the stepwise route (qf_isomp, qf_isomp_continue per step); forcing: inside qf_isomp_hooked,
    where the hook runs in the middle of an iteration.  The outer run equals the run whose hook does nothing, and every
    inner result equals the same call made outside any hook."""
    W0, dt, steps = skew(N, 0), 0.25 * qfa.hbar(N), 4
    nest = inner(N)

    def cb(W, dW):
        nest()

    def strang(h, W):
        nest()
        return W

    def forcing(P, W):
        nest()
        return force(P, W)

    busy, idle, calls = {"callback": ({"callback": cb}, {"callback": noop}, steps),
                         "strang_splitting": ({"strang_splitting": strang}, {"strang_splitting": lambda h, W: W}, 2 * steps),
                         "forcing": ({"forcing": forcing}, {"forcing": force}, None)}[route]
    Wa, sa = run_isomp(qfa, W0, dt, steps, **busy)
    made = len(nest.seen)
    Wb, sb = run_isomp(qfa, W0, dt, steps, **idle)
    print("%s N=%d: %d inner rounds, stats %s / %s, max|dW| = %.3e" % (route, N, made, sa, sb, float(np.abs(Wa - Wb).max())))
    if calls is None:      # one forcing evaluation per iteration
        calls = int(round(sa["iterations"] * steps))
    nest.check(calls)
    assert sa == sb and same(Wa, Wb), (route, N, sa, sb, float(np.abs(Wa - Wb).max()))
    assert not same(Wa, W0)


@pytest.mark.parametrize("route", ["strang_splitting", "forcing"])
@pytest.mark.parametrize("N", NESTED_SIZES)
def test_nested_heun_against_the_oracle(qfa, oracle, N, route):
    """strang_splitting = a forced heun half step (the device's heun in the device run, the oracle's in the oracle run); and on
    the qf_isomp_hooked route a forcing whose body also runs a forced heun step on an unrelated V.  State within STEP_TOL,
    iteration and maxit counts identical; on the oracle alone no step ends by maxit."""
    W0, dt, steps = skew(N, 0), 0.25 * qfa.hbar(N), 3
    V = skew(N, 7)
    if route == "strang_splitting":
        kw_dev = {"strang_splitting": lambda h, W: qfa.heun(W, h, 1, forcing=force)}
        kw_cpu = {"strang_splitting": lambda h, W: oracle.heun(W, h, 1, forcing=force)}
    else:
        def forcing(P, W):
            qfa.heun(V.copy(), dt / 2, 1, forcing=force)
            return force(P, W)
        kw_dev, kw_cpu = {"forcing": forcing}, {"forcing": force}
    sc = {"iterations": 0.0}
    Wc = oracle.isomp_fixedpoint(W0.copy(), dt, steps, stats=sc, **kw_cpu)
    Wg, sg = run_isomp(qfa, W0, dt, steps, **kw_dev)
    err = float(np.abs(Wg - Wc).max())
    print("%s N=%d: err = %.3e   err/bar = %.3e   device %s   oracle %s" % (route, N, err, err / STEP_TOL, sg, sc))
    assert sc["number_of_maxit"] == 0.0 and sc["iterations"] >= 2.0, sc
    assert sg["iterations"] == sc["iterations"] and sg["number_of_maxit"] == sc["number_of_maxit"], (sg, sc)
    assert err <= STEP_TOL, (route, N, err)
