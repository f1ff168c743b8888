"""GPU tests of the complex64 stepper's control paths and of its float32 kernels at their size-class boundaries.

tests/test_hip_single.py pins the complex64 path at the reference fixtures' sizes and default options.  This file covers
what it leaves open: the float `k_solve` at every layout switch (and under QUFLOW_HIP_SOLVE_FOLD), the first product's
tile rule (`qf_c64_tile_first`) on both sides of its thresholds, the triangle second product beyond 2048, the two-kernel
step end (compsum / reinitialize), minit / maxit / explicit tol, chained calls, `qf_c64_isomp_continue` (the carried
increment), a residual that turns non-finite mid-call, and stepper runs above N = 2048.

Every stepper comparison has two references: the oracle on the same complex64 input (the reference's own float32
arithmetic) and the oracle on that input cast to complex128 (the high-precision trajectory).  The bars are those of
test_hip_single.py: state within 1e-5 of the state's scale against the first, 2e-5 against the second, tol_auto to
rtol 1e-6, identical iteration counts (compsum: within 0.5 per step, see test_compsum_and_reinitialize_vs_oracle).
"""
import ctypes
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
SQRT_FLT_MAX = float(np.sqrt(np.finfo(np.float32).max))


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.complex128) - np.asarray(b, dtype=np.complex128))))


def make_W0_c64(oracle, N, seed):
    return oracle.make_W0(N, seed).astype(np.complex64)


def assert_skew(W):
    assert np.array_equal(W, -W.conj().T)


def expected_solve_kernel(N, fold_env=None):
    """The float k_solve layout the skew-Hermitian solve takes (csrc/poisson.hip, pick_cfg / fold_wanted): chunks of
    4 / 8 / 16 entries while one wavefront scans the walk (N <= 256 / 512 / 1024), 32 above; folded walk slots of 9 / 17
    entries (N + 1 <= 1152 / <= 2176) from N = 768 on (QUFLOW_HIP_SOLVE_FOLD=1: from 256, =0: never)."""
    fold = N + 1 <= 17 * 128 and (N >= 768 if fold_env is None else (fold_env == "1" and N >= 256))
    if fold:
        return "k_solve<float, L=%d, skew-Hermitian, folded walk slots>" % (9 if N + 1 <= 9 * 128 else 17)
    L = 4 if (N + 3) // 4 <= 64 else 8 if (N + 7) // 8 <= 64 else 16 if (N + 15) // 16 <= 64 else 32
    return "k_solve<float, L=%d, skew-Hermitian>" % L


def stepper_plan(qfa, W0, dt=None, steps=1):
    """The plan of a one-step complex64 stepper run on its own context (a solve-only call records no plan)."""
    N = W0.shape[-1]
    tr = qfa.DeviceTrajectory(W0)
    try:
        tr.advance(0.25 * qfa.hbar(N) if dt is None else dt, steps)
        return tr.ctx.plan()
    finally:
        tr.ctx.close()


def check_against_references(Wg, Wo, W64, N):
    """The state bars of test_hip_single.py: float32 oracle 1e-5, complex128 trajectory 2e-5 of the state's scale."""
    assert Wg.dtype == np.complex64
    e1 = maxabs(Wg, Wo) / np.abs(Wo).max()
    e2 = maxabs(Wg, W64) / np.abs(W64).max()
    assert e1 <= 1e-5, (N, e1)
    assert e2 <= 2e-5, (N, e2)
    assert_skew(Wg)


# ============================================================================= A. float32 kernels at their rule boundaries
SOLVE_SIZES = [253, 254, 505, 506, 767, 768, 769, 1025, 1151, 1152, 1153, 2175, 2176, 2177, 3072, 4096, 8192]


def _solve_vs_references(qfa, oracle, N, seed=11, general=False):
    """The float32 solve of the device against the double-precision solve of the same complex64 input, with the rule of
    test_solve_poisson_c64_vs_oracle_large: within `4 N eps32` of the data scale, or within twice the float32 oracle's own
    error where that is larger, and within twice that of the float32 oracle.  (From N ~ 1150 the reference's sequential
    float32 Thomas sweeps exceed 4 N eps32 themselves -- seed 11: 5.1 N eps32 at 1153, 30 N at 2177, 254 N at 8192, the
    conditioning kappa ~ N^2 / 2 of the tridiagonal systems -- so there the oracle sets the bar.)  The general branch has
    no float32 oracle: against the complex128 general solve within 2 * 4 N eps32, as test_solve_poisson_c64_vs_oracle_large,
    at sizes up to 1153 -- beyond, the same conditioning takes it past that bound (22 N eps32 at 2177) with no float32
    reference to scale the bar by."""
    W = make_W0_c64(oracle, N, seed)
    bound = 4 * N * EPS32
    if general:
        A = (W + 0.5 * np.triu(W, 1)).astype(np.complex64)
        old_d, old_o = qfa.laplacian.select_skewherm(False), oracle.select_skewherm(False)
        try:
            Pg = qfa.solve_poisson(A).copy()
            Pg_ref = oracle.solve_poisson(A.astype(np.complex128)).copy()
        finally:
            qfa.laplacian.select_skewherm(old_d)
            oracle.select_skewherm(old_o)
        assert Pg.dtype == np.complex64
        assert maxabs(Pg, Pg_ref) <= 2 * bound * np.abs(Pg_ref).max(), (N, maxabs(Pg, Pg_ref) / (EPS32 * np.abs(Pg_ref).max()))
        return A
    P_dev = qfa.solve_poisson(W).copy()
    P_ora = oracle.solve_poisson(W).copy()
    P_f64 = oracle.solve_poisson(W.astype(np.complex128)).copy()
    assert P_dev.dtype == np.complex64
    scale = np.abs(P_f64).max()
    e_dev, e_ora = maxabs(P_dev, P_f64) / scale, maxabs(P_ora, P_f64) / scale
    bar = max(bound, 2 * e_ora)
    assert e_dev <= bar, (N, e_dev / EPS32, e_ora / EPS32)
    assert maxabs(P_dev, P_ora) / scale <= 2 * max(bound, e_ora), (N, e_dev / EPS32, e_ora / EPS32)
    if N <= 1024:
        assert e_ora <= bound, (N, e_ora / EPS32)
    assert_skew(P_dev)
    return W


@pytest.mark.parametrize("N", SOLVE_SIZES)
def test_float_solve_at_layout_boundaries(qfa, oracle, N):
    """Float k_solve on both sides of every layout switch (chunk length 4 / 8 / 16 / 32, folded slots 9 / 17 and their end
    at N + 1 = 2176) up to the largest context, against the complex128 solve and the float32 oracle; the layout that ran
    is read from the plan of a one-step stepper run on the same input; the general branch at a subset of the sizes."""
    from quflow_amd.context import release_contexts
    try:
        W = _solve_vs_references(qfa, oracle, N)
        if N in (254, 506, 769, 1153):       # (the general branch: see _solve_vs_references)
            _solve_vs_references(qfa, oracle, N, seed=12, general=True)
        release_contexts()
        plan = stepper_plan(qfa, W)
        assert plan["laplacian_inverse"]["kernel"] == expected_solve_kernel(N), (N, plan["laplacian_inverse"])
    finally:
        release_contexts()


@pytest.mark.parametrize("fold", ["0", "1"])
@pytest.mark.parametrize("N", [256, 333, 1000, 1536, 2047])
def test_float_solve_fold_switch(qfa, oracle, monkeypatch, N, fold):
    """QUFLOW_HIP_SOLVE_FOLD=0 / 1 (read per launch): the walk-per-slot and the folded layouts at sizes where the default
    takes the other one, same bounds; the plan names the layout the switch asks for."""
    from quflow_amd.context import release_contexts
    monkeypatch.setenv("QUFLOW_HIP_SOLVE_FOLD", fold)
    try:
        W = _solve_vs_references(qfa, oracle, N)
        plan = stepper_plan(qfa, W)
        assert plan["laplacian_inverse"]["kernel"] == expected_solve_kernel(N, fold), (N, fold, plan["laplacian_inverse"])
    finally:
        release_contexts()


FIRST_TILE = {832: 32, 896: 64, 960: 64, 992: 32, 1088: 32, 2048: 64, 2112: 64, 2176: 64, 2304: 32, 3072: 64, 4096: 64}


def _cgemm_within_bound(N):
    """qf_cgemm at N with the operand structure and the bound of test_cgemm_vs_numpy."""
    from quflow_amd import _lib
    from quflow_amd.context import Context, ptr
    rng = np.random.default_rng(N)
    A = (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))).astype(np.complex64)
    B = (rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))).astype(np.complex64)
    B[:, 0] = 0
    A[1, :] *= 3
    C = np.zeros((N, N), dtype=np.complex64)
    ctx = Context(N)
    try:
        _lib.check(ctx._lib.qf_cgemm(ctx.handle, ptr(A), ptr(B), ptr(C)))
    finally:
        ctx.close()
    ref = A.astype(np.complex128) @ B.astype(np.complex128)
    bound = 4 * EPS32 * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)).max() * np.sqrt(N)
    assert maxabs(C, ref) <= bound, maxabs(C, ref) / bound
    assert np.all(C[:, 0] == 0)


@pytest.mark.parametrize("N", sorted(FIRST_TILE))
def test_cgemm_at_the_tile_rule(qfa, oracle, N):
    """qf_cgemm on both sides of qf_c64_tile_first (64 x 64 tiles for N % 64 == 0 with 896 <= N <= 1024, and from 2048 on
    where the tiles fill >= 85 % of their rounds of 256: 2112 just above, 2304 below), with the operand structure and the
    bound of test_cgemm_vs_numpy; the tile the stepper's first product used at that N, from its plan."""
    _cgemm_within_bound(N)
    plan = stepper_plan(qfa, make_W0_c64(oracle, N, 1))
    assert plan["first_product"]["tile"][0] == FIRST_TILE[N], (N, plan["first_product"])


# N: (kernel, tile, threads) of the plain first product on 256 CUs.  K groups (qf_launch_cgemm): exact tilings only; four
# groups of 256 threads up to one tile per CU, two up to two tiles per CU, halved until every group gets an even number of
# K-tiles of 16 ((N / 16) % (2 groups) == 0).
K_GROUP_RULE = {
    64: ("k_cgemm32<plain, 2 K groups>", 32, 512),       # 4 K-tiles: 4 groups impossible, 2 fit
    96: ("k_cgemm32<plain>", 32, 256),                   # 6 K-tiles divide by neither 8 nor 4
    100: ("k_cgemm32<plain>", 32, 256),                  # guarded tiling: never grouped
    128: ("k_cgemm32<plain, 4 K groups>", 32, 1024),     # smallest 4-group case
    544: ("k_cgemm32<plain>", 32, 256),                  # 289 tiles -> 2 groups wanted, 34 K-tiles refuse
    576: ("k_cgemm32<plain, 2 K groups>", 32, 512),      # 324 tiles, between one and two per CU
    736: ("k_cgemm32<plain>", 32, 256),                  # 529 tiles > 2 per CU
    896: ("k_cgemm_ks<4>", 64, 1024),
    960: ("k_cgemm_ks<2>", 64, 512),                     # 60 K-tiles: 8 does not divide
    1024: ("k_cgemm_ks<4>", 64, 1024),
    2048: ("k_cgemm<plain>", 64, 256),                   # four tiles per CU
}


@pytest.mark.parametrize("N", sorted(K_GROUP_RULE))
def test_cgemm_k_group_rule(qfa, oracle, N):
    """The K-group rule of the plain complex64 product, from the plan of a one-step run: which kernel, tile and workgroup
    size the first product takes at sizes on both sides of every clause of the rule, and qf_cgemm at that size within the
    bound of test_cgemm_vs_numpy (the grouped 32 x 32 variants at their smallest sizes)."""
    plan = stepper_plan(qfa, make_W0_c64(oracle, N, 1))["first_product"]
    assert (plan["kernel"], plan["tile"][0], plan["threads"]) == K_GROUP_RULE[N], (N, plan)
    _cgemm_within_bound(N)


# ============================================================================= B. stepper options against the oracle
OPTION_SIZES = [64, 100, 333, 512, 768, 1000, 1024, 1056]


def _steps(N):
    return 4 if N <= 512 else 3


def _run_both(qfa, oracle, W0, dt, steps, **kw):
    sg, so = {"iterations": 0.0}, {"iterations": 0.0}
    Wg = qfa.isomp(W0.copy(), dt, steps=steps, stats=sg, **kw)
    Wo = oracle.isomp(W0.copy(), dt, steps=steps, stats=so, **kw)
    W64 = oracle.isomp(W0.astype(np.complex128), dt, steps=steps, **kw)
    return Wg, sg, Wo, so, W64


@pytest.mark.parametrize("opt", ["compsum", "reinitialize"])
@pytest.mark.parametrize("N", OPTION_SIZES)
def test_compsum_and_reinitialize_vs_oracle(qfa, oracle, N, opt):
    """The two-kernel step end (k_norm_decide, the update kernel, the full second product) with the Kahan-compensated
    update (compsum) and with the iteration vector restarted every step (reinitialize), against both references.
    reinitialize: iteration counts equal the oracle's.  compsum: its automatic tolerance is eps32 * dt / hbar * |W| --
    the exit threshold sits at float32 rounding itself, where the device's and the reference's residuals (two float32
    evaluations) differ by their own noise, so a step may close one iteration apart: within 0.5 iterations per step, the
    slack test_isomp_c64_reference_vectors justifies against the reference's own runs; number_of_maxit equal."""
    W0 = make_W0_c64(oracle, N, 21)
    dt = 0.25 * qfa.hbar(N)
    steps = _steps(N)
    Wg, sg, Wo, so, W64 = _run_both(qfa, oracle, W0, dt, steps, **{opt: True})
    check_against_references(Wg, Wo, W64, N)
    np.testing.assert_allclose(sg["tol_auto"], so["tol_auto"], rtol=1e-6)
    slack = 0.5 if opt == "compsum" else 0.0
    assert abs(sg["iterations"] - so["iterations"]) <= slack, (sg["iterations"], so["iterations"])
    assert sg["number_of_maxit"] == so["number_of_maxit"]


def _option_kwargs(qfa, W0, dt, which):
    N = W0.shape[-1]
    if which == "minit3":
        return {"minit": 3, "maxit": 3}
    if which == "exhaust":
        return {"tol": 1e-30, "maxit": 4}
    # an explicit tol between the compensated (eps32) and the plain (sqrt(eps32)) automatic one: their geometric mean
    nrm = float(np.linalg.norm(W0, np.inf))
    return {"tol": float(EPS32 ** 0.75 * dt / qfa.hbar(N) * nrm)}


@pytest.mark.parametrize("which", ["minit3", "exhaust", "tol"])
@pytest.mark.parametrize("N", OPTION_SIZES)
def test_iteration_options_vs_oracle(qfa, oracle, monkeypatch, N, which):
    """minit = maxit = 3 (fixed iteration count), tol = 1e-30 with maxit = 4 (every step exhausts maxit) and an explicit
    tol between the two automatic ones, against both references, identical counts and number_of_maxit; then the fused
    and the two-kernel protocols (QUFLOW_HIP_FUSED=1 / 0, the full second product in both) on the same options: the same
    bits, counts and tolerance."""
    from quflow_amd.context import release_contexts
    W0 = make_W0_c64(oracle, N, 22)
    dt = 0.25 * qfa.hbar(N)
    steps = _steps(N)
    kw = _option_kwargs(qfa, W0, dt, which)
    Wg, sg, Wo, so, W64 = _run_both(qfa, oracle, W0, dt, steps, **kw)
    check_against_references(Wg, Wo, W64, N)
    assert sg["iterations"] == so["iterations"], (sg["iterations"], so["iterations"])
    assert sg["number_of_maxit"] == so["number_of_maxit"]
    assert "tol_auto" not in sg or which == "minit3"
    if which == "minit3":
        assert sg["iterations"] == 3.0
        np.testing.assert_allclose(sg["tol_auto"], so["tol_auto"], rtol=1e-6)
    if which == "exhaust":
        assert sg["iterations"] == 4.0 and sg["number_of_maxit"] == 1.0
    out = {}
    monkeypatch.setenv("QUFLOW_HIP_GEMM2", "full")
    try:
        for fused in ("1", "0"):
            monkeypatch.setenv("QUFLOW_HIP_FUSED", fused)
            release_contexts()
            st = {"iterations": 0.0}
            W = qfa.isomp(W0.copy(), dt, steps=steps, stats=st, **kw)
            tr = qfa.DeviceTrajectory(W0)
            a = tr.advance(dt, steps, **{k: v for k, v in kw.items()})
            out[fused] = (W, st["iterations"], st["number_of_maxit"], st.get("tol_auto"), tr.download(), a["total_iterations"],
                          a["number_of_maxit"], a["tol"])
            tr.ctx.close()
    finally:
        release_contexts()
    for x, y in zip(out["1"], out["0"]):
        if isinstance(x, np.ndarray):
            np.testing.assert_array_equal(x, y)
        else:
            assert x == y


@pytest.mark.parametrize("N", [100, 512, 768, 1024])
def test_chained_calls_vs_oracle(qfa, oracle, N):
    """Host-array calls of 3, 1 and 4 steps (dW restarts at every call, isospectral.py:430) against the oracle's chain of
    calls of the same lengths, counts and tolerance call by call; DeviceTrajectory.advance chunks of the same lengths
    bit-identical to the host-array chain.  N = 100: no multiple of 32 (guarded edge tiles)."""
    W0 = make_W0_c64(oracle, N, 23)
    dt = 0.25 * qfa.hbar(N)
    Wg, Wo, W64 = W0.copy(), W0.copy(), W0.astype(np.complex128)
    tr = qfa.DeviceTrajectory(W0)
    try:
        for n in (3, 1, 4):
            sg, so = {"iterations": 0.0}, {"iterations": 0.0}
            qfa.isomp(Wg, dt, steps=n, stats=sg)
            oracle.isomp(Wo, dt, steps=n, stats=so)
            oracle.isomp(W64, dt, steps=n)
            assert sg["iterations"] == so["iterations"] and sg["number_of_maxit"] == so["number_of_maxit"], n
            np.testing.assert_allclose(sg["tol_auto"], so["tol_auto"], rtol=1e-6)
            a = tr.advance(dt, n)
            assert a["total_iterations"] / n == sg["iterations"]
            np.testing.assert_array_equal(tr.download(), Wg)
        check_against_references(Wg, Wo, W64, N)
    finally:
        tr.ctx.close()


@pytest.mark.parametrize("N,steps", [(2304, 2), (3072, 2), (4096, 1)])
def test_isomp_c64_beyond_2048(qfa, oracle, N, steps):
    """The complex64 stepper above N = 2048 (a warm-started second step at 2304 and 3072; the oracle's float32 and
    complex128 steps at 4096 cost seconds each): state, counts and tolerance against both references; the plan names the
    chunk-32 solve and the first-product tile of qf_c64_tile_first."""
    from quflow_amd.context import release_contexts
    W0 = make_W0_c64(oracle, N, 24)
    dt = 0.25 * qfa.hbar(N)
    tr = qfa.DeviceTrajectory(W0)
    try:
        st = tr.advance(dt, steps)
        Wg = tr.download()
        plan = tr.ctx.plan()
    finally:
        tr.ctx.close()
    so = {"iterations": 0.0}
    Wo = oracle.isomp(W0.copy(), dt, steps=steps, stats=so)
    W64 = oracle.isomp(W0.astype(np.complex128), dt, steps=steps)
    check_against_references(Wg, Wo, W64, N)
    assert st["iterations"] == so["iterations"] and st["number_of_maxit"] == so["number_of_maxit"]
    np.testing.assert_allclose(st["tol"], so["tol_auto"], rtol=1e-6)
    assert plan["laplacian_inverse"]["kernel"] == "k_solve<float, L=32, skew-Hermitian>"
    assert plan["first_product"]["tile"][0] == FIRST_TILE[N]
    assert plan["second_product"]["kernel"].startswith("k_cgemm_tri32")
    sg = {"iterations": 0.0}
    Wh = qfa.isomp(W0.copy(), dt, steps=steps, stats=sg)
    np.testing.assert_array_equal(Wh, Wg)
    release_contexts()


# ============================================================================= C. qf_c64_isomp_continue
def _c64_call(tr, fn, dt, steps, tol, minit=1, maxit=10, compsum=0, reinitialize=0):
    from quflow_amd import _lib
    st = _lib.IsompStats()
    _lib.check(fn(tr.ctx.handle, float(dt), int(steps), float(tol), int(minit), int(maxit), int(compsum), int(reinitialize),
                  ctypes.byref(st)))
    return st


@pytest.mark.parametrize("variant", ["tri", "full", "reinitialize"])
@pytest.mark.parametrize("N", [64, 768, 1000])
def test_isomp_c64_continue_is_one_reference_call(qfa, oracle, monkeypatch, N, variant):
    """qf_c64_isomp(1 step), then qf_c64_isomp_continue(1 step) m - 1 times, is ONE reference call of m steps: the
    increment dW carries between the calls (with the triangle product dW holds only its upper tiles until the exit
    mirrors it).  The tolerance is the oracle's automatic one, passed explicitly as the reference fixes it once per call.
    reinitialize restarts dW every step and must not carry: equal to m separate one-step calls, bit for bit."""
    from quflow_amd.context import release_contexts
    m = 5
    W0 = make_W0_c64(oracle, N, 25)
    dt = 0.25 * qfa.hbar(N)
    reinit = variant == "reinitialize"
    so = {"iterations": 0.0}
    Wo = oracle.isomp(W0.copy(), dt, steps=m, stats=so, reinitialize=reinit)
    W64 = oracle.isomp(W0.astype(np.complex128), dt, steps=m, reinitialize=reinit)
    tol = float(so["tol_auto"])
    if variant == "full":
        monkeypatch.setenv("QUFLOW_HIP_GEMM2", "full")
    try:
        tr = qfa.DeviceTrajectory(W0)
        try:
            sts = [_c64_call(tr, tr._lib.qf_c64_isomp, dt, 1, tol, reinitialize=reinit)]
            for _ in range(m - 1):
                sts.append(_c64_call(tr, tr._lib.qf_c64_isomp_continue, dt, 1, tol, reinitialize=reinit))
            Wg = tr.download()
            plan = tr.ctx.plan()
        finally:
            tr.ctx.close()
        check_against_references(Wg, Wo, W64, N)
        assert sum(s.total_iterations for s in sts) / m == so["iterations"]
        assert sum(s.number_of_maxit for s in sts) / m == so["number_of_maxit"]
        if variant == "tri":
            assert plan["second_product"]["kernel"].startswith("k_cgemm_tri32"), plan["second_product"]
        if reinit:
            tr = qfa.DeviceTrajectory(W0)
            try:
                sep = [_c64_call(tr, tr._lib.qf_c64_isomp, dt, 1, tol, reinitialize=1) for _ in range(m)]
                np.testing.assert_array_equal(tr.download(), Wg)
                assert [s.total_iterations for s in sep] == [s.total_iterations for s in sts]
            finally:
                tr.ctx.close()
    finally:
        release_contexts()


# ============================================================================= D. a non-finite residual on complex64
def _oracle_residual_peaks(oracle, W0, dt, states, **kw):
    """Largest |dW_old - dW| entry of every step of the oracle's minit = maxit = 1 run, restated from its states in the
    same float32 operations (one iteration per step, dW carried from step to step: isospectral.py:475-534)."""
    vareps = dt / (2 * oracle.hbar(W0.shape[-1]))
    peaks, dW, W = [], np.zeros_like(W0), W0
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for Wn in states + [None]:
            Wh = W + dW
            P = oracle.solve_poisson(Wh).copy()
            P *= np.float32(vareps)
            PW = P @ Wh
            dWn = PW @ P + (PW - PW.conj().T)
            peaks.append(float(np.nanmax(np.abs((dW - dWn).astype(np.complex128)))))
            if Wn is None:
                break
            dW, W = dWn, Wn
    return peaks


@pytest.mark.parametrize("N,kw", [(64, {}), (512, {}), (1024, {}), (64, {"compsum": True})])
def test_nonfinite_residual_mid_call_c64(qfa, oracle, N, kw):
    """complex64 form of test_nonfinite_residual_mid_call_keeps_the_last_completed_step (dt = 1e7 hbar, one unconverged
    iteration per step): the device raises ValueError("... infs or NaNs"), writes no NaN and leaves the state of m >= 1
    completed steps of the float32 oracle.
    Where both stop: the oracle's norm (numpy abs, float32 row sums) overflows where a residual row sum passes FLT_MAX;
    the device's residual entries (sqrtf(er^2 + ei^2), row sums in double) overflow where an entry passes
    sqrt(FLT_MAX) = 1.8e19.  So the device stops in the oracle's step -- `aligned`, m = the oracle's count -- exactly when
    no completed step of the oracle had a residual entry above sqrt(FLT_MAX); otherwise it stops in the first step that
    had one (restated here from the oracle's states), still after a completed step.  A step whose completed update is
    not finite in float32 is not compared (the device cannot end on it: it writes no NaN).
    Then: the host-array entry leaves the caller's array untouched, the same context runs two ordinary steps against the
    oracle, and its plan names the triangle second product again (the skew check dropped by the abort was redone)."""
    from quflow_amd.context import release_contexts
    W0 = make_W0_c64(oracle, N, 0)
    dt = 1e7 * qfa.hbar(N)
    opts = dict(minit=1, maxit=1, **kw)
    states = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for m in range(1, 12):
            Wc = W0.copy()
            try:
                oracle.isomp(Wc, dt, steps=m, **opts)
            except ValueError as e:
                assert "infs or NaNs" in str(e)
                break
            states.append(Wc)
    assert 1 <= len(states) <= 9
    finite = [bool(np.isfinite(s).all()) for s in states]
    peaks = _oracle_residual_peaks(oracle, W0, dt, states)
    over = [k for k, p in enumerate(peaks[:len(states)]) if p > SQRT_FLT_MAX]
    near = any(SQRT_FLT_MAX / 4 < p < 4 * SQRT_FLT_MAX for p in peaks[:len(states)])     # (too close to call)
    expect_m = over[0] if over else len(states)        # steps completed before the first step the device closes
    aligned = not over
    tr = qfa.DeviceTrajectory(W0)
    try:
        with pytest.raises(ValueError, match="infs or NaNs"):
            tr.advance(dt, 12, **opts)
        Wg = tr.download()
        assert np.isfinite(Wg).all()
        assert_skew(Wg)
        rel = [maxabs(Wg, Wm) / np.abs(Wm).max() if ok else np.inf for Wm, ok in zip(states, finite)]
        m = int(np.argmin(rel)) + 1
        assert rel[m - 1] <= 1e-5, (rel, [float(np.abs(Wm).max()) for Wm in states], float(np.abs(Wg).max()))
        assert m >= 1
        if not near:
            assert m == expect_m, (m, expect_m, peaks)
            if aligned:
                assert m == len(states)
        # the context keeps working: a fresh state, two ordinary steps against the oracle
        tr.upload(W0)
        dt0 = 0.25 * qfa.hbar(N)
        s = tr.advance(dt0, 2)
        sc = {"iterations": 0.0}
        Wo = oracle.isomp(W0.copy(), dt0, steps=2, stats=sc)
        W64 = oracle.isomp(W0.astype(np.complex128), dt0, steps=2)
        check_against_references(tr.download(), Wo, W64, N)
        assert s["iterations"] == sc["iterations"] and s["number_of_maxit"] == sc["number_of_maxit"]
        assert tr.ctx.plan()["second_product"]["kernel"].startswith("k_cgemm_tri32")
    finally:
        tr.ctx.close()
    Wh = W0.copy()
    with pytest.raises(ValueError, match="infs or NaNs"):
        qfa.isomp(Wh, dt, steps=12, **opts)
    np.testing.assert_array_equal(Wh, W0)
    release_contexts()


# ============================================================================= E. a failing member of a multi call
def _diverging_ensemble_W0s(oracle, N, k, bad, dtype):
    """k initial states, member `bad` scaled by 4e7: a W scaled by s moves like one advanced with dt * s, so under the shared
    dt = 0.25 hbar that member takes the dt = 1e7 hbar path of the non-finite tests while the others step normally."""
    W0s = [oracle.make_W0(N, 70 + r).astype(dtype) for r in range(k)]
    W0s[bad] = (W0s[bad] * 4e7).astype(dtype)
    return W0s


@pytest.mark.parametrize("dtype", [np.complex128, np.complex64])
@pytest.mark.parametrize("N,k,bad", [(64, 3, 1), (512, 3, 1), (64, 6, 1), (512, 6, 2)])
def test_multi_call_with_a_failing_member(qfa, oracle, N, k, bad, dtype):
    """DeviceEnsemble.advance (qf_isomp_multi / qf_c64_isomp_multi in groups of four) with one member whose residual turns
    non-finite: every group is advanced and every member runs to its end, then ONE ValueError names the failed member and
    carries the per-member stats.  The failed member holds, bit for bit, what its own DeviceTrajectory run leaves on the
    same failure; every other member is bit-identical to its single run of all steps (k = 6: the second group too, after a
    failure in the first).  A further advance after uploading fresh states matches single runs."""
    dt = 0.25 * qfa.hbar(N)
    steps = 12
    W0s = _diverging_ensemble_W0s(oracle, N, k, bad, dtype)
    ens = qfa.DeviceEnsemble(W0s)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(ValueError, match="infs or NaNs") as exc:
                ens.advance(dt, steps, maxit=1)
        assert exc.value.failed == [bad]
        assert len(exc.value.stats) == k and exc.value.stats[bad]["failed"]
        got = ens.download()
        for r in range(k):
            tr = qfa.DeviceTrajectory(W0s[r])
            try:
                if r == bad:
                    with pytest.raises(ValueError, match="infs or NaNs"):
                        tr.advance(dt, steps, maxit=1)
                    assert np.isfinite(got[r]).all()
                else:
                    s = tr.advance(dt, steps, maxit=1)
                    st = exc.value.stats[r]
                    assert (st["total_iterations"], st["number_of_maxit"], st["tol"]) == (s["total_iterations"], s["number_of_maxit"], s["tol"])
                np.testing.assert_array_equal(got[r], tr.download())
            finally:
                tr.ctx.close()
        # fresh states: the contexts work again and match single runs
        fresh = [oracle.make_W0(N, 80 + r).astype(dtype) for r in range(k)]
        for m, W in zip(ens.members, fresh):
            m.upload(W)
        sts = ens.advance(dt, 3)
        got = ens.download()
        for r in range(k):
            tr = qfa.DeviceTrajectory(fresh[r])
            try:
                s = tr.advance(dt, 3)
                np.testing.assert_array_equal(got[r], tr.download())
                assert sts[r]["total_iterations"] == s["total_iterations"] and sts[r]["tol"] == s["tol"]
            finally:
                tr.ctx.close()
    finally:
        ens.close()
