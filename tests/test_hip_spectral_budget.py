"""GPU tests of the per-degree spectral budget: qf_spectral_budget / qf_degree_spectrum behind
quflow_amd.analysis.spectral_budget, DeviceTrajectory.spectral_budget / .enstrophy_spectrum / .energy_spectrum and
DeviceStackTrajectory.spectral_budget -- Z_l, T_l, I_l from ONE sweep of the quantization basis (k_block_vecmat_multi,
k_degree_sums).

What is an equality and what is a bound:
  * the coefficient columns omega, a, f are the existing transform's, bit for bit (the shared row loop), P is solve_poisson's;
  * the degree sums are held against numpy's sum of the same products under the worst case of two summation orders of
    2l+1 terms, 2 (2l+1) eps sum|u v|;
  * A against numpy's commutator under the product bound of tests/test_hip_parity.py::test_zgemm_vs_numpy times 2/hbar;
  * sum_l T_l (and, for the built-in Hamiltonian, sum_l T_l / (l (l+1))) vanish as well as the CPU oracle's do.

Data: W = shr2mat(omega_0), omega_0 standard normal from a seeded default_rng, omega_0[0] = 0, degree l damped by
(l (l+1))^0.75; forcing AffineForcing(F0, a_W=-0.5, a_P=0.3, a_lap=2e-5) with F0 random, exactly skew-Hermitian,
max|F0| = 2 max|W|.  Sizes 33 (odd, one edge tile), 64, 100, 257 (the blocks of 257 and 1 rows cross the vecmat's 256-row
LDS chunk); 1024 with lmax = 256 for many blocks and several 64-column groups per block."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SIZES = [33, 64, 100, 257]
A_W, A_P, A_LAP = -0.5, 0.3, 2e-5


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


# ----------------------------------------------------------------------------- data (made once, read only)
_DATA = {}


def _cached(key, make):
    if key not in _DATA:
        a = make()
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        _DATA[key] = a
    return _DATA[key]


def degrees(n):
    return np.floor(np.sqrt(np.arange(n))).astype(np.int64)


def omega0(N, zonal=False):
    def make():
        rng = np.random.default_rng(1000 + N)
        om = rng.standard_normal(N * N)
        om[0] = 0.0
        l = degrees(N * N)[1:].astype(np.float64)
        om[1:] /= (l * (l + 1)) ** 0.75
        if zonal:
            keep = np.zeros(N * N, dtype=bool)
            ll = np.arange(N)
            keep[ll * ll + ll] = True
            om[~keep] = 0.0
        return om
    return _cached(("omega0", N, zonal), make)


def state(qfa, N, zonal=False):
    def make():
        # (above the other tests' sizes the basis is built slab by slab: same bits, no N^3/3 host copy for this module)
        W = qfa.shr2mat(omega0(N, zonal), N, streamed=True if N > 512 else None)
        assert np.array_equal(W, -W.conj().T)
        return W
    return _cached(("W", N, zonal), make)


def pattern(qfa, N):
    def make():
        rng = np.random.default_rng(2000 + N)
        B = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        F0 = B - B.conj().T
        F0 = F0 * (2 * np.abs(state(qfa, N)).max() / np.abs(F0).max())
        assert np.array_equal(F0, -F0.conj().T)
        return F0
    return _cached(("F0", N), make)


def forcing(qfa, N):
    return _cached(("forcing", N), lambda: qfa.AffineForcing(pattern(qfa, N), a_W=A_W, a_P=A_P, a_lap=A_LAP))


def ctx_mat2shr(ctx, M, nmax):
    """qf_mat2shr on `ctx` band-limited to nmax, of the host matrix M (None: the context's resident state)."""
    from quflow_amd import _lib
    from quflow_amd.context import ptr
    om = np.zeros(nmax * nmax, dtype=np.float64)
    Mc = None if M is None else np.ascontiguousarray(M, dtype=np.complex128)
    _lib.check(ctx._lib.qf_mat2shr(ctx.handle, None if Mc is None else ptr(Mc), ptr(om), ctypes.c_longlong(nmax * nmax)))
    return om


def buffer(ctx, name):
    from quflow_amd import _lib
    from quflow_amd.context import ptr
    out = np.empty((ctx.N, ctx.N), dtype=np.complex128)
    _lib.check(ctx._lib.qf_download_buffer(ctx.handle, _lib.BUFFER_IDS[name], ptr(out)))
    return out


def slab_mb(N):
    """A slab budget of two and a half of the largest block (N x N doubles): a full transform takes about N / 7.5 slabs."""
    return 2.5 * 8 * N * N / 2.0 ** 20


def run_budget(qfa, N, form, lmax, monkeypatch, with_forcing=True, zonal=False, hamiltonian=None):
    """(budget with coefficients, the context it ran on, A, P, keep-alive) for one of the three forms: 'host' (host in, resident
    basis), 'streamed' (host in, slabs) and 'state' (a DeviceTrajectory's resident state)."""
    from quflow_amd.quantization import _transform_context
    W = state(qfa, N, zonal)
    f = forcing(qfa, N) if with_forcing else None
    if form == "state":
        tr = qfa.DeviceTrajectory(W, forcing=f, hamiltonian=hamiltonian)
        b = tr.spectral_budget(lmax=lmax, coefficients=True)
        ctx = tr.ctx
    else:
        if form == "streamed":
            monkeypatch.setenv("QUFLOW_HIP_BASIS_SLAB_MB", repr(slab_mb(N)))
        streamed = form == "streamed"
        b = qfa.analysis.spectral_budget(W, hamiltonian=hamiltonian, forcing=f, lmax=lmax, coefficients=True, streamed=streamed)
        ctx = _transform_context(N, None, streamed)
        tr = None
    return b, ctx, buffer(ctx, "PW"), buffer(ctx, "Phalf"), tr


def check_columns(qfa, N, b, ctx, A, P, nmax, host_W):
    W = state(qfa, N)
    c = b["coefficients"]
    assert np.array_equal(c["omega"], ctx_mat2shr(ctx, W if host_W else None, nmax))
    assert np.array_equal(c["tendency"], ctx_mat2shr(ctx, A, nmax))
    assert np.array_equal(c["forcing"], ctx_mat2shr(ctx, forcing(qfa, N)(P, W), nmax))
    assert np.any(c["tendency"] != 0.0) and np.any(c["forcing"] != 0.0)


def degree_sum_errors(b, nmax):
    """For each row (name, device values for l = 1..nmax-1, u, v): the largest error against numpy's sum of u v over the
    degree in units of the bound 2 (2l+1) eps sum|u v|."""
    c = b["coefficients"]
    rows = [("Z", b["enstrophy"], c["omega"], c["omega"]), ("T", b["enstrophy_transfer"] / 2, c["omega"], c["tendency"])]
    if "forcing" in c:
        rows.append(("I", b["enstrophy_input"] / 2, c["omega"], c["forcing"]))
    out = {}
    for name, dev, u, v in rows:
        worst = 0.0
        prod = u * v
        for l in range(1, nmax):
            sl = slice(l * l, (l + 1) * (l + 1))
            bound = 2 * (2 * l + 1) * EPS * np.abs(prod[sl]).sum()
            err = abs(dev[l - 1] - prod[sl].sum())
            assert err <= bound, (name, l, dev[l - 1], prod[sl].sum(), err, bound)
            if bound > 0:
                worst = max(worst, err / bound)
        out[name] = worst
    return out


# ----------------------------------------------------------------------------- 1. the columns are the existing transform
@pytest.mark.parametrize("half_band", [False, True])
@pytest.mark.parametrize("form", ["host", "streamed", "state"])
@pytest.mark.parametrize("N", SIZES)
def test_columns_are_mat2shr_bit_for_bit(qfa, monkeypatch, N, form, half_band):
    nmax = N // 2 if half_band else N
    if form == "streamed" and N == 100:
        from quflow_amd import _lib
        n = _lib.load().qf_basis_slab_plan(N, nmax, ctypes.c_longlong(int(slab_mb(N) * 2 ** 20)), None, 0)
        assert n >= 3, n
    b, ctx, A, P, _tr = run_budget(qfa, N, form, nmax if half_band else None, monkeypatch)
    assert b["el"].shape == (nmax - 1,) and b["coefficients"]["omega"].shape == (nmax * nmax,)
    check_columns(qfa, N, b, ctx, A, P, nmax, host_W=form != "state")


# ----------------------------------------------------------------------------- 2. A is the bracket, P the solve
@pytest.mark.parametrize("form", ["host", "state"])
@pytest.mark.parametrize("N", SIZES)
def test_tendency_is_the_bracket(qfa, monkeypatch, N, form):
    W = state(qfa, N)
    _b, _ctx, A, P, _tr = run_budget(qfa, N, form, None, monkeypatch)
    assert np.array_equal(P, qfa.solve_poisson(W))
    hb = qfa.hbar(N)
    ref = (P @ W - W @ P) / hb
    bound = 8 * EPS * N * (np.abs(P) @ np.abs(W)).max() * (2 / hb)
    err = np.abs(A - ref).max()
    print("N=%d %s: max|A - [P,W]/hbar| = %.3e, bound %.3e" % (N, form, err, bound))
    assert err <= bound, (err, bound)
    assert np.array_equal(A, -A.conj().T)


# ----------------------------------------------------------------------------- 3. the degree sums
@pytest.mark.parametrize("form", ["host", "streamed", "state"])
@pytest.mark.parametrize("N", SIZES)
def test_degree_sums(qfa, monkeypatch, N, form):
    b, _ctx, _A, _P, _tr = run_budget(qfa, N, form, None, monkeypatch)
    worst = degree_sum_errors(b, N)
    print("N=%d %s: worst error / bound per row: %s" % (N, form, worst))
    assert set(worst) == {"Z", "T", "I"}


@pytest.mark.parametrize("N", SIZES)
def test_trajectory_spectra(qfa, N):
    tr = qfa.DeviceTrajectory(state(qfa, N))
    om = tr.shr()
    el, Z = tr.enstrophy_spectrum()
    el_ref, Z_ref = qfa.analysis.enstrophy_spectrum(om)
    assert np.array_equal(el, el_ref) and Z.shape == Z_ref.shape
    sq = np.abs(om * om)
    bound = np.array([2 * (2 * l + 1) * EPS * sq[l * l:(l + 1) * (l + 1)].sum() for l in range(1, N)])
    assert np.all(np.abs(Z - Z_ref) <= bound), np.abs((Z - Z_ref) / bound).max()
    for beta in (0, 1):
        el, E = tr.energy_spectrum(beta=beta)
        el_ref, E_ref = qfa.analysis.energy_spectrum(om, beta=beta)
        assert np.array_equal(el, el_ref)
        assert np.all(np.abs(E - E_ref) <= bound / (el * (el + 1)) ** (1 - beta / 2))
    # the normalisation: sum Z_l / 2 is the enstrophy, sum Z_l / (l (l+1)) / 2 the energy
    energy, enstrophy = tr.diagnostics()
    assert abs(Z.sum() / 2 - enstrophy) <= 64 * N * EPS * enstrophy
    assert abs(tr.energy_spectrum()[1].sum() / 2 - energy) <= 64 * N * EPS * abs(energy)


# ----------------------------------------------------------------------------- 4. conservation
def defects(el, omega, a, T, nmax):
    """(enstrophy defect, energy defect): |sum_l T_l w_l| / sum_l 2 sum_m |omega a| w_l for w_l = 1 and 1 / (l (l+1))."""
    absprod = np.abs(omega * a)
    den = np.array([2 * absprod[l * l:(l + 1) * (l + 1)].sum() for l in range(1, nmax)])
    ll = (el * (el + 1)).astype(np.float64)
    return abs(T.sum()) / den.sum(), abs((T / ll).sum()) / (den / ll).sum()


def oracle_defects(oracle, qfa, N, offset=None):
    from oracle import quantization_oracle as qo
    W = np.array(state(qfa, N))
    P = oracle.solve_poisson((W if offset is None else W - offset).copy()).copy()
    A = (P @ W - W @ P) / qfa.hbar(N)
    om, a = qo.mat2shr(W), qo.mat2shr(A)
    el = np.arange(1, N)
    prod = om * a
    T = np.array([2 * prod[l * l:(l + 1) * (l + 1)].sum() for l in range(1, N)])
    return defects(el, om, a, T, N)


@pytest.mark.parametrize("N", SIZES)
def test_transfer_sums_to_zero(qfa, oracle, monkeypatch, N):
    b, _ctx, _A, _P, _tr = run_budget(qfa, N, "state", None, monkeypatch, with_forcing=False)
    c = b["coefficients"]
    dz, de = defects(b["el"], c["omega"], c["tendency"], b["enstrophy_transfer"], N)
    oz, oe = _cached(("oracle_defects", N), lambda: oracle_defects(oracle, qfa, N))
    biggest = np.abs(b["enstrophy_transfer"]).max() / (2 * np.abs(c["omega"] * c["tendency"]).sum())
    print("N=%d: device defects %.3e (enstrophy) %.3e (energy); oracle %.3e %.3e; N eps %.3e; largest |T_l| / denominator %.3e"
          % (N, dz, de, oz, oe, N * EPS, biggest))
    assert np.array_equal(b["energy_transfer"], b["enstrophy_transfer"] / (b["el"] * (b["el"] + 1)))
    assert dz <= 4 * max(oz, N * EPS), (dz, oz)
    assert de <= 4 * max(oe, N * EPS), (de, oe)


@pytest.mark.parametrize("N", SIZES)
def test_transfer_sums_to_zero_with_coriolis(qfa, oracle, monkeypatch, N):
    offset = qfa.coriolis(N, 0.5)
    ham = qfa.TridiagonalHamiltonian.poisson(N, offset=offset)
    for form in ("state", "host"):
        b, _ctx, _A, P, _tr = run_budget(qfa, N, form, None, monkeypatch, with_forcing=False, hamiltonian=ham)
        assert np.array_equal(P, ham(state(qfa, N)))
        c = b["coefficients"]
        dz, _ = defects(b["el"], c["omega"], c["tendency"], b["enstrophy_transfer"], N)
        oz, _ = _cached(("oracle_defects_coriolis", N), lambda: oracle_defects(oracle, qfa, N, offset))
        print("N=%d %s, coriolis: device enstrophy defect %.3e; oracle %.3e" % (N, form, dz, oz))
        assert dz <= 4 * max(oz, N * EPS), (dz, oz)


# ----------------------------------------------------------------------------- 5. a zonal state does not move
@pytest.mark.parametrize("form", ["host", "state"])
@pytest.mark.parametrize("N", SIZES)
def test_zonal_state(qfa, monkeypatch, N, form):
    W = state(qfa, N, zonal=True)
    assert np.count_nonzero(W - np.diag(np.diag(W))) == 0 and np.count_nonzero(W) > 0
    b, _ctx, A, P, _tr = run_budget(qfa, N, form, None, monkeypatch, with_forcing=False, zonal=True)
    assert np.count_nonzero(P - np.diag(np.diag(P))) == 0
    assert np.count_nonzero(A) == 0
    assert np.all(b["enstrophy_transfer"] == 0.0) and np.all(b["energy_transfer"] == 0.0)
    assert np.all(b["enstrophy_flux"] == 0.0)
    # Z_l is the square of the one coefficient of its degree (the transform's omega_l0; every m != 0 entry is zero)
    om = b["coefficients"]["omega"]
    l = np.arange(1, N)
    only = np.zeros(N * N, dtype=bool)
    only[np.arange(N) ** 2 + np.arange(N)] = True
    assert np.count_nonzero(om[~only]) == 0
    ref = om[l * l + l] ** 2
    assert np.all(np.abs(b["enstrophy"] - ref) <= 4 * EPS * ref)


# ----------------------------------------------------------------------------- 6. nothing is disturbed
def forced_pair(qfa, N, make_forcing):
    W = state(qfa, N)
    visc = qfa.ViscDampStep(nu=2e-5, alpha=0.5)
    return [qfa.DeviceTrajectory(W, forcing=make_forcing(), strang_splitting=visc) for _ in range(2)], visc


@pytest.mark.parametrize("N", [33, 64])
def test_budget_leaves_a_forced_run_alone(qfa, N):
    dt = 0.25 * qfa.hbar(N)
    (tr, ref), visc = forced_pair(qfa, N, lambda: forcing(qfa, N))
    s1 = tr.advance(dt, 3)
    W_mid = tr.download()
    b = tr.spectral_budget()
    assert np.array_equal(tr.download(), W_mid)
    s2 = tr.advance(dt, 3)
    r1 = ref.advance(dt, 3)
    r2 = ref.advance(dt, 3)
    assert np.array_equal(tr.download(), ref.download())
    assert s1 == r1 and s2 == r2
    # the host-in call gives the resident call's numbers
    h = qfa.analysis.spectral_budget(W_mid, forcing=forcing(qfa, N), strang_splitting=visc)
    assert sorted(h) == sorted(b)
    for key in b:
        assert np.array_equal(h[key], b[key]), key
    assert {"enstrophy_input", "energy_input", "enstrophy_dissipation", "energy_dissipation"} <= set(b)


@pytest.mark.parametrize("N", [33, 64])
def test_budget_leaves_a_stochastic_run_alone(qfa, N):
    dt = 0.25 * qfa.hbar(N)
    make = lambda: qfa.StochasticForcing(2, 6, 0.05, seed=7, a_W=A_W, a_P=A_P, a_lap=A_LAP, step=11)
    (tr, ref), _visc = forced_pair(qfa, N, make)
    s1 = tr.advance(dt, 3)
    step = tr.forcing.step
    assert step == 14 and tr.stochastic_tell() == 14
    b = tr.spectral_budget(coefficients=True)
    assert tr.forcing.step == step and tr.stochastic_tell() == step
    # the affine terms alone: the pattern of the last step does not enter
    W, P = tr.download(), buffer(tr.ctx, "Phalf")
    affine = qfa.AffineForcing(a_W=A_W, a_P=A_P, a_lap=A_LAP)
    assert np.array_equal(b["coefficients"]["forcing"], ctx_mat2shr(tr.ctx, affine(P, W), N))
    s2 = tr.advance(dt, 3)
    r1 = ref.advance(dt, 3)
    r2 = ref.advance(dt, 3)
    assert np.array_equal(tr.download(), ref.download())
    assert s1 == r1 and s2 == r2 and tr.forcing.step == ref.forcing.step == 17


def test_stack_member_budget(qfa):
    N = 33
    W = state(qfa, N)
    stack = np.stack([W, 0.5 * W])
    st = qfa.DeviceStackTrajectory(stack)
    b0, b1 = st.spectral_budget(0), st.spectral_budget(1, lmax=17)
    ref = qfa.DeviceTrajectory(W).spectral_budget()
    for key in ref:
        assert np.array_equal(b0[key], ref[key]), key
    assert np.array_equal(b1["enstrophy"], 0.25 * ref["enstrophy"][:16])
    assert np.array_equal(st.download(), stack)


# ----------------------------------------------------------------------------- 7. the host arithmetic
def test_flux_and_dissipation_arithmetic(qfa):
    N = 64
    nu, alpha = 2e-5, 0.5
    tr = qfa.DeviceTrajectory(state(qfa, N), forcing=forcing(qfa, N), strang_splitting=qfa.ViscDampStep(nu=nu, alpha=alpha))
    b = tr.spectral_budget()
    el = b["el"]
    ll = (el * (el + 1)).astype(np.float64)
    assert np.array_equal(el, np.arange(1, N))
    assert np.array_equal(b["energy"], b["enstrophy"] / ll)
    assert np.array_equal(b["energy_transfer"], b["enstrophy_transfer"] / ll)
    assert np.array_equal(b["energy_input"], b["enstrophy_input"] / ll)
    assert np.array_equal(b["enstrophy_flux"], -np.cumsum(b["enstrophy_transfer"]))
    assert np.array_equal(b["energy_flux"], -np.cumsum(b["energy_transfer"]))
    assert np.array_equal(b["enstrophy_dissipation"], -2 * (nu * ll + alpha) * b["enstrophy"])
    assert np.array_equal(b["energy_dissipation"], b["enstrophy_dissipation"] / ll)
    T = b["enstrophy_transfer"]
    assert abs(b["enstrophy_flux"][-1] + T.sum()) <= N * EPS * np.abs(T).sum()
    assert "coefficients" not in b


# ----------------------------------------------------------------------------- 8. refusals
def test_refusals(qfa):
    from quflow_amd import _lib, integrators
    from quflow_amd.context import ptr
    N = 33
    W = state(qfa, N)
    tr = qfa.DeviceTrajectory(W)
    for bad in (1, 0, -3, N + 1):
        with pytest.raises(ValueError):
            tr.spectral_budget(lmax=bad)
        with pytest.raises(ValueError):
            qfa.analysis.spectral_budget(W, lmax=bad)
    out = np.zeros((3, N))
    lib = tr.ctx._lib
    tr._need_basis()
    for bad in (1, N + 1):
        assert lib.qf_spectral_budget(tr.ctx.handle, None, bad, ptr(out), None) == 1          # QF_ERR_INVALID
        assert lib.qf_degree_spectrum(tr.ctx.handle, None, bad, ptr(out)) == 1
    assert lib.qf_spectral_budget(tr.ctx.handle, None, N, None, None) == 1
    integrators.select_skewherm(False)
    try:
        with pytest.raises(NotImplementedError):
            tr.spectral_budget()
        with pytest.raises(NotImplementedError):
            qfa.analysis.spectral_budget(W)
    finally:
        integrators.select_skewherm(True)
    assert np.array_equal(tr.download(), W)
    W32 = W.astype(np.complex64)
    single = qfa.DeviceTrajectory(W32)
    assert single.c64
    for call in (single.spectral_budget, single.enstrophy_spectrum, single.energy_spectrum):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError):
        qfa.analysis.spectral_budget(W32)
    _lib.check(lib.qf_basis_compute(single.ctx.handle))
    assert lib.qf_spectral_budget(single.ctx.handle, None, N, ptr(out), None) == 4             # QF_ERR_STATE
    assert np.array_equal(single.download(), W32)


# ----------------------------------------------------------------------------- 9. many blocks, several column groups
def test_large_band_limited(qfa, monkeypatch):
    N, nmax = 1024, 256
    b, ctx, A, P, _tr = run_budget(qfa, N, "state", nmax, monkeypatch)
    check_columns(qfa, N, b, ctx, A, P, nmax, host_W=False)
    worst = degree_sum_errors(b, nmax)
    print("N=%d lmax=%d: worst error / bound per row: %s" % (N, nmax, worst))
