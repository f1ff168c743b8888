"""Rotations, gradients and initial data on the MI355X: quflow_amd.geometry (rotation_matrix, rotate, grad),
quflow_amd.dynamics (north_blob, blob, project_el), physics.sectional_curvature, quantization.elmr2mat / elmc2mat and
DeviceTrajectory.rotate / .grad.

The rotation's tolerance is tests/test_geometry_host.py's rot_tol: entrywise 8 N max(1, |xi|) eps max|entry|.  Every case
prints its worst error in units of N max(1, |xi|) eps max|entry| (the bar is 8).

Sizes of the rotation tests, N = 2, 5, 33, 64, 257, 1024: a Taylor window clipped at both matrix edges (N smaller than one
32-column strip plus 2 d rows), guarded 32 x 32 product tiles, the 32 x 32 product path, a size that is no multiple of 32, and
the pipelined 64 x 64 product path; the gradient's workgroups cover 8 rows x 256 columns, so 257 and 1024 take more than one
of them in both directions.
"""
import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import linalg
from test_geometry_host import EPS, XIS, FIXTURE_SIZES, gen, golden, rot_tol, rodrigues   # noqa: F401  (golden: fixture)

pytestmark = pytest.mark.gpu

SIZES = (2, 5, 33, 64, 257, 1024)
Z_SIZES = (2, 5, 64, 257, 1024)


def report(what, N, xi, err, scale=1.0):
    unit = N * max(1.0, float(np.linalg.norm(xi))) * EPS * scale
    print("%-40s N=%5d |xi|=%.3f  max err = %.3e   err/(N max(1,|xi|) eps scale) = %.3f" % (what, N, np.linalg.norm(xi), err, err / unit))
    assert err <= 8.0 * unit, (what, N, err, 8.0 * unit)


def maxabs(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max())


def skew_state(N, salt=51):
    """A skew-Hermitian state with entries of order 1 / N (a vorticity-like scale at which the stepper converges)."""
    return gen.skewherm(N, salt) / N


# ---- 1-3: the rotation matrix -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_rotation_matrix_against_reference(golden, N):
    for i, xi in enumerate(XIS):
        R = qfa.rotation_matrix(xi, N)
        assert R.dtype == np.complex128 and R.shape == (N, N)
        report("rotation_matrix vs expm", N, xi, maxabs(R, golden["expm_%d_%d" % (i, N)]))


@pytest.mark.parametrize("N", Z_SIZES)
def test_pure_z_rotation_and_unitarity(N):
    a = np.arange(N) - (N - 1) / 2
    for xi3 in (2.5, -0.4):
        xi = np.array([0.0, 0.0, xi3])
        R = qfa.rotation_matrix(xi, N)
        report("z rotation vs diag(exp(i xi3 (a-s)))", N, xi, maxabs(R, np.diag(np.exp(1j * xi3 * a))))
    for xi in XIS:
        R = qfa.rotation_matrix(xi, N)
        report("|R R^H - I|", N, xi, maxabs(R @ R.conj().T, np.eye(N)))


def test_zero_and_full_turn():
    for N in (5, 16):
        assert np.array_equal(qfa.rotation_matrix(np.zeros(3), N), np.eye(N))      # sigma = 0, d = 1: I + 0 exactly
        xi = 2 * np.pi * np.array([2.0, -1.0, 2.0]) / 3.0                           # |xi| = 2 pi, not reduced
        want = np.eye(N) * (-1.0 if N % 2 == 0 else 1.0)
        report("full turn = (-1)^(N-1) I", N, xi, maxabs(qfa.rotation_matrix(xi, N), want))


# ---- 4: equivariance ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", SIZES)
def test_equivariance(N):
    """rotate(xi, S_j) = sum_i Q_ij S_i with Q the Rodrigues matrix of xi: needs no fixture, pins every sign end to end."""
    S = qfa.so3_generators(N)
    for xi in (XIS if N < 1024 else XIS[:1]):
        Q = rodrigues(xi)
        for j in range(3):
            want = sum(Q[k, j] * S[k] for k in range(3))
            report("rotate(xi, S_%d)" % (j + 1), N, xi, maxabs(qfa.rotate(xi, S[j]), want), np.abs(S[j]).max())


# ---- 5-7: rotate --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_rotate_against_reference(golden, N):
    data = gen.inputs(N)
    for kind in ("generic", "skew"):
        W = data["W_" + kind]
        for i, xi in enumerate(XIS):
            out = qfa.rotate(xi, W)
            assert out is not W and out.dtype == np.complex128
            ref = golden["rotate_%s_%d_%d" % (kind, i, N)]
            report("rotate %s vs reference" % kind, N, xi, maxabs(out, ref), np.abs(ref).max())
    W32 = data["W_generic"].astype(np.complex64)
    out = qfa.rotate(XIS[0], W32)
    assert out.dtype == np.complex64
    # complex64 in, computed in double, complex64 out: the rounding of the input (eps32 |W|_F <= eps32 N max|W| through a
    # unitary map) and of the result
    assert maxabs(out, golden["rotate_generic_0_%d" % N]) <= 2 * np.finfo(np.float32).eps * np.abs(W32).max() * N


@pytest.mark.parametrize("N", (5, 33, 257))
def test_rotate_back(N):
    W = gen.generic(N, 61)
    for xi in XIS:
        mid = qfa.rotate(xi, W)
        back = qfa.rotate(-xi, mid)
        # two rotations: twice the bar, against the largest entry either of the two results has
        report("rotate(-xi, rotate(xi, W)) = W", N, xi, maxabs(back, W) / 2, max(np.abs(W).max(), np.abs(mid).max()))


def test_rotation_preserves_invariants():
    N = 257
    W = skew_state(N)
    Wr = qfa.rotate(XIS[1], W)

    def rel(a, b):
        return abs(a - b) / abs(a)
    assert rel(qfa.norm_L2(W), qfa.norm_L2(Wr)) <= 1e-11
    assert rel(qfa.enstrophy(W), qfa.enstrophy(Wr)) <= 1e-11
    assert rel(qfa.energy_euler(W), qfa.energy_euler(Wr)) <= 1e-11            # the Laplacian commutes with rotations
    # Wr and Wr^H are each within the bar of the exact, skew-Hermitian, rotated matrix (the eigensolver wants N eps)
    Wr_skew = (Wr - Wr.conj().T) / 2
    assert maxabs(Wr, Wr_skew) <= rot_tol(N, XIS[1], np.abs(Wr).max())
    lam = linalg.eig_skewherm(W, vectors=False)
    lam_r = linalg.eig_skewherm(Wr_skew, vectors=False)
    assert np.abs(lam - lam_r).max() <= 1e-11 * np.abs(lam).max()


# ---- 8: grad ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_grad_against_reference(golden, N):
    P = gen.inputs(N)["P"]
    dP = qfa.grad(P)
    ref = golden["grad_%d" % N]
    assert dP.shape == (3, N, N) and dP.dtype == np.complex128
    # the reference's own error: six dense products of hbar S_k (|S_k| <= N/2) and P, divided by hbar
    assert maxabs(dP, ref) <= 16 * N * EPS * np.abs(P).max() * N / 2
    assert qfa.grad(P.astype(np.complex64)).dtype == np.complex64


@pytest.mark.parametrize("N", (33, 257, 1024))
def test_grad_against_device_bracket(N):
    P = gen.generic(N, 63)
    dP = qfa.grad(P)
    X = qfa.cartesian_generators(N)
    for k in range(3):
        ref = qfa.bracket(X[k], P)
        err = maxabs(dP[k], ref)
        print("grad[%d] vs bracket  N=%5d  max err = %.3e   err/(N eps max|P|) = %.3f"
              % (k, N, err, err / (N * EPS * np.abs(P).max())))
        assert err <= 16 * N * EPS * np.abs(P).max()


@pytest.mark.parametrize("N", (15, 16, 64))
def test_hoppe_yau_laplacian(N):
    rng = np.random.default_rng(N)
    P = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    P -= P.conj().T
    W = np.zeros_like(P)
    for k in range(3):
        W += qfa.grad(qfa.grad(P)[k])[k]
    np.testing.assert_allclose(W, qfa.laplace(P))          # the reference's test_hoppe_yau_laplacian: rtol 1e-7


@pytest.mark.parametrize("N", (2, 3))
def test_grad_edges(N):
    P = gen.generic(N, 65)
    S = qfa.so3_generators(N)
    dP = qfa.grad(P)
    for k in range(3):
        want = S[k] @ P - P @ S[k]
        for name, sl in (("first row", np.s_[0, :]), ("last row", np.s_[-1, :]), ("first column", np.s_[:, 0]),
                         ("last column", np.s_[:, -1]), ("all", np.s_[:, :])):
            assert maxabs(dP[k][sl], want[sl]) <= 8 * EPS * np.abs(P).max() * N, (k, name)


# ---- 9: the resident state ----------------------------------------------------------------------------------------------

def test_trajectory_rotate_and_grad_bits():
    N = 64
    W0 = skew_state(N)
    xi = XIS[0]
    traj = qfa.DeviceTrajectory(W0)
    assert traj.rotate(xi) is traj
    Wr = traj.download()
    assert np.array_equal(Wr, qfa.rotate(xi, W0))
    assert np.array_equal(traj.grad(), qfa.grad(Wr))


@pytest.mark.parametrize("N", (64, 1024))
def test_trajectory_rotate_then_advance(N):
    """The carried-increment rule: a trajectory that has stepped (so that it carries an increment, buffer parities and the
    knowledge that W is skew-Hermitian), is rotated in place and steps on equals, bit for bit, a fresh trajectory that starts
    from the rotated matrix."""
    dt = 0.25 * qfa.hbar(N)
    traj = qfa.DeviceTrajectory(skew_state(N))
    traj.advance(dt, 2)
    W1 = traj.download()
    traj.rotate(XIS[0])
    W1r = traj.download()
    assert np.array_equal(W1r, qfa.rotate(XIS[0], W1))
    s1 = traj.advance(dt, 3)
    fresh = qfa.DeviceTrajectory(W1r)
    s2 = fresh.advance(dt, 3)
    assert s1["total_iterations"] == s2["total_iterations"]
    assert np.array_equal(traj.download(), fresh.download())


def test_trajectory_complex64_is_refused():
    """Double only: a single-precision trajectory refuses (where complex64 states are kept in double, it simply works)."""
    traj = qfa.DeviceTrajectory(skew_state(16).astype(np.complex64))
    if traj.c64:
        with pytest.raises(NotImplementedError):
            traj.rotate(XIS[0])
        with pytest.raises(NotImplementedError):
            traj.grad()
    else:
        assert traj.rotate(XIS[0]).grad().shape == (3, 16, 16)


# ---- 10: initial data, curvature, basis elements ------------------------------------------------------------------------

@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_blobs_against_reference(golden, N):
    assert np.array_equal(qfa.north_blob(N, 0), golden["north_blob_s0_%d" % N])
    nb = qfa.north_blob(N, 0.1)
    heat_tol = 16 * N * EPS * np.abs(nb).max()          # one diagonally dominant tridiagonal solve per diagonal
    assert maxabs(nb, golden["north_blob_s01_%d" % N]) <= heat_tol
    for i, pos in enumerate(gen.BLOB_POS):
        ref = golden["blob_%d_%d" % (i, N)]
        xi = qfa.dynamics.rotation_vector(pos)
        err = maxabs(qfa.blob(N, np.array(pos), 0.1), ref)
        print("blob at %s  N=%d  max err = %.3e  (max entry %.3e)" % (pos, N, err, np.abs(ref).max()))
        # the rotation's bar, plus the rounding of xi itself (a few eps |xi|, times |S|_2 <= N / 2), plus the heat solve
        assert err <= (rot_tol(N, xi) + 2 * N * EPS * np.linalg.norm(xi)) * np.abs(nb).max() + heat_tol


@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_sectional_curvature_against_reference(golden, N):
    """Relative 1e-10 on pairs that are linearly independent (gen.curvature_pairs says why they have to be: for a nearly
    parallel pair the expression's Poisson terms cancel to 1e-8 of themselves and the reference's own last digits are
    noise).  Here the largest term is at most 11 times the result, so the bar leaves some 1e4 roundings of room."""
    ref = golden["curvature_%d" % N]
    for i, (F, G) in enumerate(gen.inputs(N)["pairs"]):
        C = qfa.sectional_curvature(F, G)
        print("sectional_curvature N=%d pair %d: %.15e  reference %.15e  rel %.2e" % (N, i, C, ref[i], abs(C - ref[i]) / abs(ref[i])))
        assert abs(C - ref[i]) <= 1e-10 * abs(ref[i])


@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_basis_elements_against_reference(golden, N):
    for el, m in gen.elm_cases(N):
        for name, fn in (("elmr", qfa.elmr2mat), ("elmc", qfa.elmc2mat)):
            T = fn(el, m, N)
            assert T.el == el and T.shape == (N, N) and T.format == "dia"
            # the device basis agrees with the reference's LAPACK one to 1e-12 (tests/test_hip_parity.py)
            assert maxabs(T.toarray(), golden["%s_%d_%d_%d" % (name, el, m, N)]) <= 1e-12, (name, el, m)
        assert abs(qfa.norm_L2(qfa.elmr2mat(el, m, N).toarray()) - 1) <= 1e-12


# ---- 11: project_el -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", FIXTURE_SIZES)
def test_project_el(golden, N):
    data = gen.inputs(N)
    for kind in ("generic", "skew"):
        W = data["W_" + kind]
        tol = 1e-12 * np.abs(W).max()
        for el in gen.PROJECT_ELS:
            tag = gen.el_tag(el)
            PW = qfa.project_el(W, el)
            QW = qfa.project_el(W, el, complement=True)
            assert maxabs(qfa.project_el(PW, el), PW) <= tol                    # a projection: idempotent
            assert maxabs(qfa.project_el(PW, el, complement=True), 0 * PW) <= tol
            assert maxabs(PW + QW, W) <= tol
            # the documented factor: the reference returns N P_el W, and W - N P_el W as the "complement"
            ref = golden["project_%s_el%s_c0_%d" % (kind, tag, N)]
            ref_c = golden["project_%s_el%s_c1_%d" % (kind, tag, N)]
            err = maxabs(N * PW, ref)
            print("N project_el(%s W, el=%s)  N=%d  max err = %.3e  (bar %.3e)" % (kind, tag, N, err, tol))
            assert err <= tol
            assert maxabs(W - N * PW, ref_c) <= tol
    assert maxabs(qfa.project_el(data["W_skew"], -1), qfa.project_el(data["W_skew"], N - 1)) == 0


# ---- 12: error paths ----------------------------------------------------------------------------------------------------

def test_error_paths_leave_the_context_usable():
    N = 16
    W = gen.generic(N, 67)
    xi = XIS[0]
    good = qfa.rotate(xi, W)
    with pytest.raises(ValueError):
        qfa.rotate(xi, W[:, :-1])
    with pytest.raises(ValueError):
        qfa.rotate(xi[:2], W)
    with pytest.raises(ValueError):
        qfa.rotation_matrix(np.zeros((3, 1)), N)
    bad_xi = xi.copy()
    bad_xi[1] = np.nan
    for call in (lambda: qfa.rotate(bad_xi, W), lambda: qfa.rotation_matrix(bad_xi, N)):
        with pytest.raises(qfa.QuflowHipError, match="INVALID"):
            call()
    bad_W = W.copy()
    bad_W[3, 5] = np.nan
    with pytest.raises(qfa.QuflowHipError, match="NONFINITE"):
        qfa.rotate(xi, bad_W)
    bad_W[3, 5] = np.inf
    with pytest.raises(qfa.QuflowHipError, match="NONFINITE"):
        qfa.grad(bad_W)
    assert np.array_equal(qfa.rotate(xi, W), good)
    assert np.all(np.isfinite(qfa.grad(W)))
    # the resident state is untouched by a refused rotation
    traj = qfa.DeviceTrajectory(W)
    with pytest.raises(qfa.QuflowHipError, match="INVALID"):
        traj.rotate(bad_xi)
    with pytest.raises(ValueError):
        traj.rotate(xi[:2])
    assert np.array_equal(traj.download(), W)
    assert np.array_equal(traj.rotate(xi).download(), good)
