"""GPU tests of the per-degree MHD budget: qf_mhd_spectral_budget behind quflow_amd.analysis.mhd_spectral_budget and
DeviceStackTrajectory.mhd_budget -- nine degree-sum rows of omega, theta and the three tendencies (advection [P,W]/hbar,
Lorentz term [B,Theta]/hbar, induction [P,Theta]/hbar) from ONE sweep of the quantization basis that carries five vectors.

What is an equality and what is a bound:
  * the five coefficient columns are the existing transform's, bit for bit (the shared row loop); P is solve_poisson's and
    B is laplace's, bit for bit; every tendency is exactly skew-Hermitian;
  * a tendency against numpy's bracket: the product bound of tests/test_hip_spectral_budget.py::test_tendency_is_the_bracket,
    8 eps N max(|X| |Y|) 2/hbar;
  * a degree sum against numpy's sum of the same products: the worst case of two summation orders of 2l+1 terms,
    2 (2l+1) eps sum|u v|; cross_helicity_transfer, the sum of three rows, the sum of their three bounds;
  * the dictionary is its formulas applied to the rows, np.array_equal;
  * the five totals against DeviceMHDTrajectory.diagnostics(): 64 N eps of each (the cross helicity, which may be near
    zero: 64 N eps sum|omega theta|);
  * the five sums that vanish: as well as the CPU oracle's do on the same pair, 4 max(oracle's defect, N eps).

Data: W as in tests/test_hip_spectral_budget.py (seed 1000 + N, degree l damped by (l (l+1))^0.75); Theta = shr2mat of
standard normals from seed 3000 + N, theta_0 = 0, damped by (l (l+1))^1.25, so that B = Delta Theta is as rough as W.
Sizes 33 (odd, one edge tile), 64, 100, 257 (blocks of 257 and 1 rows cross the sweep's 256-row LDS chunk), each full band
and lmax = N // 2, in three forms: host in (resident basis), host in streamed (slab budget of 2.5 largest blocks), and the
resident pair of a DeviceMHDTrajectory; 1024 with lmax = 256 through the streamed basis."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SIZES = [33, 64, 100, 257]
FORMS = ["host", "streamed", "resident"]
NAMES = ("omega", "theta", "advection", "lorentz", "induction")
# row r = scale_r sum_m u v: (u, v, scale)
ROWS = [("omega", "omega", 1), ("theta", "theta", 1), ("omega", "theta", 1), ("omega", "advection", 2),
        ("omega", "lorentz", 2), ("theta", "induction", 2), ("theta", "advection", 1), ("theta", "lorentz", 1),
        ("omega", "induction", 1)]


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


def coefficients0(N, seed, power, zonal=False):
    rng = np.random.default_rng(seed + N)
    om = rng.standard_normal(N * N)
    om[0] = 0.0
    l = degrees(N * N)[1:].astype(np.float64)
    om[1:] /= (l * (l + 1)) ** power
    if zonal:
        keep = np.zeros(N * N, dtype=bool)
        ll = np.arange(N)
        keep[ll * ll + ll] = True
        om[~keep] = 0.0
    return om


def pair(qfa, N, zonal=False):
    """The (2,N,N) state (W, Theta)."""
    def make():
        streamed = True if N > 512 else None
        W = qfa.shr2mat(coefficients0(N, 1000, 0.75, zonal), N, streamed=streamed)
        Theta = qfa.shr2mat(coefficients0(N, 3000, 1.25), N, streamed=streamed)
        assert np.array_equal(W, -W.conj().T) and np.array_equal(Theta, -Theta.conj().T)
        return np.stack([W, Theta])
    return _cached(("pair", N, zonal), make)


def ctx_mat2shr(ctx, M, nmax):
    """qf_mat2shr on `ctx` band-limited to nmax, of the host matrix M."""
    from quflow_amd import _lib
    from quflow_amd.context import ptr
    om = np.zeros(nmax * nmax, dtype=np.float64)
    Mc = np.ascontiguousarray(M, dtype=np.complex128)
    _lib.check(ctx._lib.qf_mat2shr(ctx.handle, ptr(Mc), ptr(om), ctypes.c_longlong(nmax * nmax)))
    return om


def buffer(ctx, name):
    from quflow_amd import _lib
    from quflow_amd.context import ptr
    out = np.empty((ctx.N, ctx.N), dtype=np.complex128)
    _lib.check(ctx._lib.qf_download_buffer(ctx.handle, _lib.MHD_BUFFER_IDS[name], ptr(out)))
    return out


def raw_rows(ctx, nmax):
    """The nine rows straight from the C entry point, for the pair that is resident on `ctx`."""
    from quflow_amd import _lib
    from quflow_amd.context import ptr
    rows = np.zeros((9, nmax), dtype=np.float64)
    _lib.check(ctx._lib.qf_mhd_spectral_budget(ctx.handle, nmax, ptr(rows), None))
    return rows


def slab_mb(N):
    """A slab budget of two and a half of the largest block (N x N doubles)."""
    return 2.5 * 8 * N * N / 2.0 ** 20


class Run:
    """One budget call with coefficients: the dictionary, the context it ran on, the five matrices it left, the raw rows."""

    def __init__(self, qfa, N, form, lmax, monkeypatch, zonal=False):
        from quflow_amd.quantization import _transform_context
        state = pair(qfa, N, zonal)
        self.N, self.nmax = N, N if lmax is None else lmax
        if form == "resident":
            self.tr = qfa.DeviceMHDTrajectory(np.array(state))
            self.b = self.tr.mhd_budget(lmax=lmax, coefficients=True)
            self.ctx = self.tr.ctx
        else:
            streamed = form == "streamed"
            if streamed:
                monkeypatch.setenv("QUFLOW_HIP_BASIS_SLAB_MB", repr(slab_mb(N)))
            self.tr = None
            self.b = qfa.analysis.mhd_spectral_budget(state, lmax=lmax, coefficients=True, streamed=streamed)
            self.ctx = _transform_context(N, None, streamed)
        self.mats = {k: buffer(self.ctx, k) for k in ("P", "B", "advection", "lorentz", "induction")}
        self.rows = raw_rows(self.ctx, self.nmax)


def row_bounds(c, nmax):
    """Per row r: (numpy's sums of u v, the bound 2 (2l+1) eps sum|u v|) for l = 1..nmax-1, both without the row's scale."""
    out = []
    for u, v, _scale in ROWS:
        prod = c[u] * c[v]
        ref = np.array([prod[l * l:(l + 1) * (l + 1)].sum() for l in range(1, nmax)])
        bound = np.array([2 * (2 * l + 1) * EPS * np.abs(prod[l * l:(l + 1) * (l + 1)]).sum() for l in range(1, nmax)])
        out.append((ref, bound))
    return out


# ----------------------------------------------------------------------------- 1. the columns are the existing transform
@pytest.mark.parametrize("half_band", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", SIZES)
def test_columns_are_mat2shr_bit_for_bit(qfa, monkeypatch, N, form, half_band):
    nmax = N // 2 if half_band else N
    if form == "streamed" and N == 100:
        from quflow_amd import _lib
        n = _lib.load().qf_basis_slab_plan(N, nmax, ctypes.c_longlong(int(slab_mb(N) * 2 ** 20)), None, 0)
        assert n >= 3, n
    r = Run(qfa, N, form, nmax if half_band else None, monkeypatch)
    c = r.b["coefficients"]
    assert sorted(c) == sorted(NAMES)
    assert r.b["el"].shape == (nmax - 1,) and all(c[k].shape == (nmax * nmax,) for k in NAMES)
    W, Theta = pair(qfa, N)
    for name, M in (("omega", W), ("theta", Theta), ("advection", r.mats["advection"]), ("lorentz", r.mats["lorentz"]),
                    ("induction", r.mats["induction"])):
        assert np.array_equal(c[name], ctx_mat2shr(r.ctx, M, nmax)), name
        assert np.any(c[name] != 0.0), name


# ----------------------------------------------------------------------------- 2. the matrices
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", SIZES)
def test_matrices(qfa, monkeypatch, N, form):
    W, Theta = pair(qfa, N)
    r = Run(qfa, N, form, None, monkeypatch)
    P, B = r.mats["P"], r.mats["B"]
    assert np.array_equal(P, qfa.solve_poisson(W))
    assert np.array_equal(B, qfa.laplace(Theta))
    hb = qfa.hbar(N)
    for name, X, Y in (("advection", P, W), ("lorentz", B, Theta), ("induction", P, Theta)):
        T = r.mats[name]
        assert np.array_equal(T, -T.conj().T), name
        ref = (X @ Y - Y @ X) / hb
        bound = 8 * EPS * N * (np.abs(X) @ np.abs(Y)).max() * (2 / hb)
        err = np.abs(T - ref).max()
        print("N=%d %s %s: max|T - bracket| = %.3e, bound %.3e" % (N, form, name, err, bound))
        assert err <= bound, (name, err, bound)


# ----------------------------------------------------------------------------- 3. the degree sums
@pytest.mark.parametrize("half_band", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", SIZES)
def test_degree_sums(qfa, monkeypatch, N, form, half_band):
    nmax = N // 2 if half_band else N
    r = Run(qfa, N, form, nmax if half_band else None, monkeypatch)
    rb = row_bounds(r.b["coefficients"], nmax)
    worst = []
    for i, (_u, _v, scale) in enumerate(ROWS):
        ref, bound = rb[i]
        err = np.abs(r.rows[i, 1:] / scale - ref)
        assert np.all(err <= bound), (i, np.max(err / np.where(bound > 0, bound, 1)))
        worst.append(float(np.max(err / np.where(bound > 0, bound, np.inf))))
    print("N=%d %s nmax=%d: worst error / bound per row: %s" % (N, form, nmax, ["%.2f" % w for w in worst]))
    ref = rb[6][0] + rb[7][0] + rb[8][0]
    bound = rb[6][1] + rb[7][1] + rb[8][1]
    assert np.all(np.abs(r.b["cross_helicity_transfer"] - ref) <= bound)


# ----------------------------------------------------------------------------- 4. the dictionary is its formulas
@pytest.mark.parametrize("half_band", [False, True])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", SIZES)
def test_dictionary(qfa, monkeypatch, N, form, half_band):
    nmax = N // 2 if half_band else N
    r = Run(qfa, N, form, nmax if half_band else None, monkeypatch)
    b, rows = r.b, r.rows[:, 1:]
    el = np.arange(1, nmax)
    ll = (el * (el + 1)).astype(np.float64)
    want = {"el": el, "enstrophy": rows[0], "kinetic_energy": rows[0] / ll, "magnetic_potential": rows[1],
            "magnetic_energy": ll * rows[1], "energy": rows[0] / ll + ll * rows[1], "cross_helicity": rows[2],
            "kinetic_transfer_advection": rows[3] / ll, "kinetic_transfer_lorentz": rows[4] / ll,
            "magnetic_transfer": ll * rows[5], "energy_transfer": rows[3] / ll + rows[4] / ll + ll * rows[5],
            "enstrophy_transfer_advection": rows[3], "enstrophy_source_lorentz": rows[4], "potential_transfer": rows[5],
            "cross_helicity_transfer": rows[6] + rows[7] + rows[8]}
    for flux, transfer in (("kinetic_flux_advection", "kinetic_transfer_advection"), ("energy_flux", "energy_transfer"),
                           ("potential_flux", "potential_transfer"), ("cross_helicity_flux", "cross_helicity_transfer"),
                           ("enstrophy_flux_advection", "enstrophy_transfer_advection")):
        want[flux] = -np.cumsum(want[transfer])
    assert set(b) == set(want) | {"coefficients"}
    for key in want:
        assert np.array_equal(b[key], want[key]), key
    assert "enstrophy_flux_lorentz" not in b          # (a source, not a transfer: no flux)


# ----------------------------------------------------------------------------- 5. the totals are the diagnostics
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", SIZES)
def test_totals_are_the_diagnostics(qfa, monkeypatch, N, form):
    r = Run(qfa, N, form, None, monkeypatch)
    d = _cached(("diagnostics", N), lambda: qfa.DeviceMHDTrajectory(np.array(pair(qfa, N))).diagnostics())
    b, c = r.b, r.b["coefficients"]
    for total, key in ((b["kinetic_energy"].sum() / 2, "energy_kinetic"), (b["magnetic_energy"].sum() / 2, "energy_magnetic"),
                       (b["magnetic_potential"].sum() / 2, "magnetic_casimir"), (b["enstrophy"].sum() / 2, "enstrophy")):
        print("N=%d %s %s: budget %.17g diagnostics %.17g" % (N, form, key, total, d[key]))
        assert abs(total - d[key]) <= 64 * N * EPS * abs(d[key]), key
    scale = np.abs(c["omega"] * c["theta"]).sum()
    print("N=%d %s cross_helicity: budget %.17g diagnostics %.17g" % (N, form, b["cross_helicity"].sum(), d["cross_helicity"]))
    assert abs(b["cross_helicity"].sum() - d["cross_helicity"]) <= 64 * N * EPS * scale


# ----------------------------------------------------------------------------- 6. conservation
def degree_abs(u, v, nmax):
    a = np.abs(u * v)
    return np.array([a[l * l:(l + 1) * (l + 1)].sum() for l in range(1, nmax)])


def defects(rows, c, nmax):
    """The five relative defects |sum T| / sum of the absolute products, from the rows l = 1..nmax-1 (9, nmax-1)."""
    el = np.arange(1, nmax)
    ll = (el * (el + 1)).astype(np.float64)
    wa = 2 * degree_abs(c["omega"], c["advection"], nmax)
    wb = 2 * degree_abs(c["omega"], c["lorentz"], nmax)
    tc = 2 * degree_abs(c["theta"], c["induction"], nmax)
    ch = (degree_abs(c["theta"], c["advection"], nmax) + degree_abs(c["theta"], c["lorentz"], nmax)
          + degree_abs(c["omega"], c["induction"], nmax))
    return {"kinetic_advection": abs((rows[3] / ll).sum()) / (wa / ll).sum(),
            "lorentz_induction": abs((rows[4] / ll + ll * rows[5]).sum()) / (wb / ll + ll * tc).sum(),
            "potential": abs(rows[5].sum()) / tc.sum(),
            "cross_helicity": abs((rows[6] + rows[7] + rows[8]).sum()) / ch.sum(),
            "enstrophy_advection": abs(rows[3].sum()) / wa.sum()}


def oracle_defects(oracle, qfa, N):
    from oracle import quantization_oracle as qo
    W, Theta = (np.array(x) for x in pair(qfa, N))
    hb = qfa.hbar(N)
    P = oracle.solve_poisson(W.copy()).copy()
    B = np.array(oracle.laplace(Theta.copy()))
    mats = {"omega": W, "theta": Theta, "advection": (P @ W - W @ P) / hb, "lorentz": (B @ Theta - Theta @ B) / hb,
            "induction": (P @ Theta - Theta @ P) / hb}
    c = {k: qo.mat2shr(M) for k, M in mats.items()}
    rows = np.empty((9, N - 1))
    for i, (u, v, scale) in enumerate(ROWS):
        prod = c[u] * c[v]
        rows[i] = [scale * prod[l * l:(l + 1) * (l + 1)].sum() for l in range(1, N)]
    return defects(rows, c, N)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", SIZES)
def test_conservation(qfa, oracle, monkeypatch, N, form):
    r = Run(qfa, N, form, None, monkeypatch)
    dev = defects(r.rows[:, 1:], r.b["coefficients"], N)
    ora = _cached(("oracle_defects", N), lambda: oracle_defects(oracle, qfa, N))
    assert set(dev) == set(ora) and len(dev) == 5
    for key in dev:
        print("N=%d %s %s: device defect %.3e, oracle %.3e, N eps %.3e" % (N, form, key, dev[key], ora[key], N * EPS))
    for key in dev:
        assert dev[key] <= 4 * max(ora[key], N * EPS), (key, dev[key], ora[key])


# ----------------------------------------------------------------------------- 7. a zonal W is not advected
@pytest.mark.parametrize("form", ["host", "resident"])
@pytest.mark.parametrize("N", SIZES)
def test_zonal_vorticity(qfa, monkeypatch, N, form):
    W = pair(qfa, N, zonal=True)[0]
    assert np.count_nonzero(W - np.diag(np.diag(W))) == 0 and np.count_nonzero(W) > 0
    r = Run(qfa, N, form, None, monkeypatch, zonal=True)
    c = r.b["coefficients"]
    assert np.count_nonzero(r.mats["advection"]) == 0
    assert np.all(c["advection"] == 0.0)
    assert np.all(r.rows[3] == 0.0) and np.all(r.rows[6] == 0.0)
    assert np.all(r.b["kinetic_transfer_advection"] == 0.0) and np.all(r.b["enstrophy_flux_advection"] == 0.0)
    for name, row in (("lorentz", 4), ("induction", 5)):
        assert np.any(c[name] != 0.0) and np.any(r.rows[row] != 0.0), name


# ----------------------------------------------------------------------------- 8. the run is left alone
@pytest.mark.parametrize("N", [33, 64])
def test_budget_leaves_the_run_alone(qfa, N):
    dt = 0.25 * qfa.hbar(N)
    state = np.array(pair(qfa, N))
    tr, ref = qfa.DeviceMHDTrajectory(state), qfa.DeviceMHDTrajectory(state)
    s1 = tr.advance(dt, 3)
    mid, d_mid = tr.download(), tr.diagnostics()
    b = tr.mhd_budget(coefficients=True)
    assert np.array_equal(tr.download(), mid)
    assert tr.diagnostics() == d_mid
    s2 = tr.advance(dt, 3)
    r1 = ref.advance(dt, 3)
    r2 = ref.advance(dt, 3)
    assert np.array_equal(tr.download(), ref.download())
    assert s1 == r1 and s2 == r2
    assert tr.diagnostics() == ref.diagnostics()
    # the host-in call gives the resident call's numbers
    h = qfa.analysis.mhd_spectral_budget(mid, coefficients=True)
    assert sorted(h) == sorted(b)
    for key in b:
        if key == "coefficients":
            assert all(np.array_equal(h[key][k], b[key][k]) for k in NAMES)
        else:
            assert np.array_equal(h[key], b[key]), key
    # the hydrodynamic budget of one member is still there, and still leaves the stack alone
    assert "enstrophy_transfer" in tr.spectral_budget(0)
    assert np.array_equal(tr.download(), ref.download())


# ----------------------------------------------------------------------------- 9. refusals
def test_refusals(qfa):
    from quflow_amd import _lib, integrators
    from quflow_amd.context import ptr
    N = 33
    state = np.array(pair(qfa, N))
    W = state[0]
    lib = _lib.load()
    out = np.zeros((9, N))
    # not the MHD pair
    three = qfa.DeviceStackTrajectory(np.stack([W, W, W]))
    plain = qfa.DeviceStackTrajectory(state.copy())
    for st in (three, plain):
        with pytest.raises(ValueError):
            st.mhd_budget()
    three._member._need_basis()
    assert lib.qf_mhd_spectral_budget(three.ctx.handle, N, ptr(out), None) == 1          # QF_ERR_INVALID: k = 3
    assert np.array_equal(three.download(), np.stack([W, W, W])) and np.array_equal(plain.download(), state)
    # no stack
    single = qfa.DeviceTrajectory(W)
    single._need_basis()
    assert lib.qf_mhd_spectral_budget(single.ctx.handle, N, ptr(out), None) == 4         # QF_ERR_STATE
    assert np.array_equal(single.download(), W)
    # bad arguments
    tr = qfa.DeviceMHDTrajectory(state)
    tr._member._need_basis()
    for bad in (1, 0, -3, N + 1):
        assert lib.qf_mhd_spectral_budget(tr.ctx.handle, bad, ptr(out), None) == 1
        with pytest.raises(ValueError):
            tr.mhd_budget(lmax=bad)
        with pytest.raises(ValueError):
            qfa.analysis.mhd_spectral_budget(state, lmax=bad)
    assert lib.qf_mhd_spectral_budget(tr.ctx.handle, N, None, None) == 1
    # a slab budget too small for block 0: refused before anything is launched
    _lib.check(lib.qf_basis_stream(tr.ctx.handle, ctypes.c_longlong(8 * N * N - 8)))
    assert lib.qf_mhd_spectral_budget(tr.ctx.handle, N, ptr(out), None) == 1
    _lib.check(lib.qf_basis_stream(tr.ctx.handle, ctypes.c_longlong(0)))
    # what is installed on the context: the system is the built-in one
    with integrators._forcing_on(tr.ctx, qfa.AffineForcing(a_W=-0.5)):
        assert lib.qf_mhd_spectral_budget(tr.ctx.handle, N, ptr(out), None) == 6         # QF_ERR_UNSUPPORTED
    with integrators._hamiltonian_on(tr.ctx, qfa.TridiagonalHamiltonian.poisson(N, offset=qfa.coriolis(N, 0.5))):
        assert lib.qf_mhd_spectral_budget(tr.ctx.handle, N, ptr(out), None) == 6
    assert np.all(out == 0.0)
    # before any of these buffers exists, there is nothing to download
    scratch = np.empty((N, N), dtype=np.complex128)
    assert lib.qf_download_buffer(tr.ctx.handle, _lib.MHD_BUFFER_IDS["P"], ptr(scratch)) == 4
    assert np.array_equal(tr.download(), state)
    # the modes and types the budget does not have
    integrators.select_skewherm(False)
    try:
        with pytest.raises(NotImplementedError):
            tr.mhd_budget()
        with pytest.raises(NotImplementedError):
            qfa.analysis.mhd_spectral_budget(state)
    finally:
        integrators.select_skewherm(True)
    with pytest.raises(NotImplementedError):
        qfa.analysis.mhd_spectral_budget(state.astype(np.complex64))
    with pytest.raises(ValueError):
        qfa.analysis.mhd_spectral_budget(W)
    # and after all that the call works, on the same context
    assert lib.qf_mhd_spectral_budget(tr.ctx.handle, N, ptr(out), None) == 0 and np.any(out != 0.0)
    assert np.array_equal(tr.download(), state)


# ----------------------------------------------------------------------------- 10. many blocks, several column groups
def test_large_band_limited(qfa, monkeypatch):
    N, nmax = 1024, 256
    r = Run(qfa, N, "streamed", nmax, monkeypatch)
    c = r.b["coefficients"]
    W, Theta = pair(qfa, N)
    for name, M in (("omega", W), ("theta", Theta), ("advection", r.mats["advection"]), ("lorentz", r.mats["lorentz"]),
                    ("induction", r.mats["induction"])):
        assert np.array_equal(c[name], ctx_mat2shr(r.ctx, M, nmax)), name
        assert np.any(c[name] != 0.0), name
    rb = row_bounds(c, nmax)
    for i, (_u, _v, scale) in enumerate(ROWS):
        ref, bound = rb[i]
        assert np.all(np.abs(r.rows[i, 1:] / scale - ref) <= bound), i
