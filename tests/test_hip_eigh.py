"""The device eigensolver (quflow_amd.linalg: eigh, eigvalsh, eig_skewherm), the spectrum of a resident trajectory and
quflow_amd.analysis.scale_decomposition on the MI355X.

Inputs, error measures and bars come from tests/test_eigh_host.py: every bar is 8 x the worst ratio numpy.linalg.eigh
reaches on that file's inputs, the same constant at every N.  Errors are evaluated on the host from what the device
returned, in long double up to N = 257 and in fp64 above.  Every case prints `max err` and `err/bar`.

Sizes: the host file's SIZES, N = 1 (read off on the host: no context is that small) and 257; the kernels have two size
classes -- both rows of a pair in registers up to N = 2048, two reads above -- so 2048 and 2049 stand on either side of
that boundary; one case at N = 1024.  The workgroup is 256 threads at every size.
"""
import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import linalg
from test_eigh_host import (EPS, CLD, SIZES, C_ORTH, C_RES, C_LAM, C_SD, C_COMM, RATIO_RES, GAP_CAP, hermitian, skew,
                            spin_case, clustered, sd_case, orth_err, res_err, comm_err, norm2, ws_from_vectors, ws_eigh_numpy)

pytestmark = pytest.mark.gpu

ALL_SIZES = (1,) + SIZES + (257,)
CLASS_SIZES = (1024, 2048, 2049)          # one inside the register class, its last size, the first of the two-read class
LD_MAX = 257


def report(what, N, err, bar):
    print("%-34s N=%5d  max err = %.3e   err/bar = %.3f" % (what, N, err, err / bar if bar > 0 else (0.0 if err == 0 else np.inf)))
    assert err <= bar, (what, N, err, bar)


def check_decomposition(H, lam, V, what, lam_exact=None):
    """The orthogonality, residual and eigenvalue bars of case 1 for a device result (lam, V) of the Hermitian H."""
    N = H.shape[0]
    ld = N <= LD_MAX
    nH = norm2(H)
    assert lam.dtype == np.float64 and V.dtype == np.complex128 and lam.shape == (N,) and V.shape == (N, N)
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(V))
    assert np.all(np.diff(lam) >= 0), "lambda is not ascending"
    report(what + ": |V^H V - I|", N, orth_err(V, ld), C_ORTH * N * EPS)
    report(what + ": |H V - V lam|", N, res_err(H, lam, V, ld), C_RES * N * EPS * nH)
    ref = np.linalg.eigvalsh(H) if lam_exact is None else lam_exact
    report(what + ": |lam - eigvalsh|", N, float(np.abs(lam - ref).max()), (C_RES + RATIO_RES) * N * EPS * nH)


# ---- 1. dense Hermitian ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("damped", [False, True], ids=["white", "damped"])
@pytest.mark.parametrize("N", ALL_SIZES)
def test_dense_hermitian(N, damped):
    H = hermitian(N, damped)
    assert N == 1 or np.abs(H.imag).max() > 0.01 * np.abs(H.real).max()     # complex entries: a missing conjugate fails
    lam, V = linalg.eigh(H)
    check_decomposition(H, lam, V, "damped" if damped else "white")


@pytest.mark.parametrize("N", CLASS_SIZES)
def test_dense_hermitian_size_classes(N):
    H = hermitian(N, False)
    lam, V = linalg.eigh(H)
    print("N=%d: %s" % (N, linalg.last_stats()))
    check_decomposition(H, lam, V, "white")


# ---- 2. known spectrum -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", ALL_SIZES)
def test_known_spectrum(N):
    W, H, exact = spin_case(N)
    bar = C_LAM * N * EPS * np.abs(exact).max()
    report("spin, eigh(H)", N, float(np.abs(linalg.eigh(H)[0] - exact).max()), bar)
    lam, V = linalg.eig_skewherm(W)
    report("spin, eig_skewherm(W)", N, float(np.abs(lam - exact).max()), bar)
    # W = V diag(i lam) V^H
    if N > 1:
        report("spin, |W V - V i lam|", N, res_err(-1j * W, lam, V), C_RES * N * EPS * norm2(H))


# ---- 3. degenerate and trivial inputs -------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [16, 65])
def test_clustered_spectrum(N):
    H, exact = clustered(N)
    lam, V = linalg.eigh(H)
    print("N=%d: %s" % (N, linalg.last_stats()))
    check_decomposition(H, lam, V, "three clusters", lam_exact=exact)


def test_trivial_matrices():
    N = 8
    d = np.array([3.0, -1.5, 0.25, 7.0, -1.5, 0.0, 2.0, -6.0])
    for name, H, exact in (("zero", np.zeros((N, N), complex), np.zeros(N)), ("diagonal", np.diag(d).astype(complex), np.sort(d)),
                           ("3 I", 3.0 * np.eye(N, dtype=complex), np.full(N, 3.0))):
        lam, V = linalg.eigh(H)
        assert np.all(np.isfinite(lam)) and np.all(np.isfinite(V)), name
        assert np.array_equal(lam, exact), (name, lam)
        report(name + ": |V^H V - I|", N, orth_err(V), C_ORTH * N * EPS)
        assert res_err(H, lam, V) == 0.0, name
        assert np.array_equal(linalg.eigvalsh(H), exact), name
    assert linalg.last_stats()["sweeps"] == 1
    linalg.eigh(np.zeros((N, N), complex))
    assert linalg.last_stats()["sweeps"] == 0


# ---- 4, 5. eigenvalues only; reproducibility ------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [5, 64, 257])
def test_eigenvalues_only_and_reproducible(N):
    H = hermitian(N, True)
    lam, V = linalg.eigh(H)
    assert linalg.eigvalsh(H).tobytes() == lam.tobytes()
    lam2, V2 = linalg.eigh(H.copy())
    assert lam2.tobytes() == lam.tobytes() and V2.tobytes() == V.tobytes()
    W = 1j * H
    assert linalg.eig_skewherm(W, vectors=False).tobytes() == linalg.eig_skewherm(W)[0].tobytes()


# ---- 6. real use: the stream matrix of a smooth state -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def smooth():
    out = {}
    for N in (64, 130):
        W = qfa.shr2mat(qfa.analysis.random_shr(lmax=N - 1, seed=100 + N))
        out[N] = (W, qfa.solve_poisson(W))
    return out


@pytest.mark.parametrize("N", [64, 130])
def test_stream_matrix_of_a_smooth_state(smooth, N):
    W, P = smooth[N]
    assert np.abs(P + P.conj().T).max() == 0.0
    lam, V = linalg.eig_skewherm(P)
    H = -1j * P
    report("smooth P: |V^H V - I|", N, orth_err(V), C_ORTH * N * EPS)
    report("smooth P: |P V - V i lam|", N, res_err(H, lam, V), C_RES * N * EPS * norm2(H))


# ---- 7. resident state ----------------------------------------------------------------------------------------------------

def test_spectrum_of_a_resident_trajectory():
    N = 64
    W0 = qfa.shr2mat(qfa.analysis.random_shr(lmax=N - 1, seed=9))
    tr = qfa.DeviceTrajectory(W0)
    lam0 = tr.spectrum()
    assert lam0.tobytes() == linalg.eig_skewherm(tr.download(), vectors=False).tobytes()
    tr.advance(0.5 * qfa.hbar(N), 20)
    lam = tr.spectrum()
    H = -1j * tr.download()
    H = (H + H.conj().T) / 2
    report("resident state after 20 steps", N, float(np.abs(lam - np.linalg.eigvalsh(H)).max()), (C_RES + RATIO_RES) * N * EPS * norm2(H))
    print("spectrum drift over 20 steps: %.3e (not asserted)" % float(np.abs(lam - lam0).max()))
    with pytest.raises(NotImplementedError):
        qfa.DeviceTrajectory(W0.astype(np.complex64)).spectrum()


# ---- 8. scale_decomposition ---------------------------------------------------------------------------------------------------

def check_properties(W, P, Ws, Wr, what):
    N = W.shape[0]
    nW, nP = norm2(W), norm2(P)
    assert Wr.tobytes() == (W - Ws).tobytes(), what
    report(what + ": |Ws + Ws^H|", N, float(np.abs(Ws + Ws.conj().T).max()), C_RES * N * EPS * nW)
    report(what + ": |P Ws - Ws P|", N, comm_err(P, Ws), C_COMM * N * EPS * nP * nW)


@pytest.mark.parametrize("N", SIZES)
def test_scale_decomposition_white(N):
    W, P, g = sd_case(N)
    assert g <= GAP_CAP
    nW = norm2(W)
    Ws, Wr = qfa.scale_decomposition(W, P)
    # (a) assembly, free of the gaps: the formula on the host, in long double, from the device's own eigenvectors
    lam, V = linalg.eig_skewherm(P)
    report("assembly from the device's V", N, float(np.abs(Ws - ws_from_vectors(W, V)).max()), C_RES * N * EPS * nW)
    # (b) independent: numpy's eigh form
    report("against numpy eigh(-iP)", N, float(np.abs(Ws - ws_eigh_numpy(W, P)).max()), C_SD * N * EPS * nW * max(1.0, g))
    # (c) properties
    check_properties(W, P, Ws, Wr, "white")


@pytest.mark.parametrize("N", [64, 130])
def test_scale_decomposition_smooth(smooth, N):
    W, P = smooth[N]
    Ws, Wr = qfa.scale_decomposition(W)                         # P = None: the device's own solve
    check_properties(W, P, Ws, Wr, "smooth")
    # (d) the same bits with P handed in
    Ws2, Wr2 = qfa.scale_decomposition(W, P=qfa.solve_poisson(W))
    assert Ws2.tobytes() == Ws.tobytes() and Wr2.tobytes() == Wr.tobytes()
    # (e) a foreign hamiltonian is honoured
    seen = []

    def helmholtz(X):
        seen.append(X.shape)
        return qfa.solve_helmholtz(X)
    Ws3, Wr3 = qfa.scale_decomposition(W, hamiltonian=helmholtz)
    assert seen == [(N, N)]
    Ws4, _ = qfa.scale_decomposition(W, P=qfa.solve_helmholtz(W))
    assert Ws3.tobytes() == Ws4.tobytes() and Ws3.tobytes() != Ws.tobytes()
    check_properties(W, qfa.solve_helmholtz(W), Ws3, Wr3, "helmholtz")
    # (f) the resident form
    tr = qfa.DeviceTrajectory(W)
    Ws5, Wr5 = tr.scale_decomposition()
    Ws6, Wr6 = qfa.scale_decomposition(tr.download())
    assert Ws5.tobytes() == Ws6.tobytes() and Wr5.tobytes() == Wr6.tobytes() and Ws5.tobytes() == Ws.tobytes()


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------

def test_errors():
    H = hermitian(16, False)
    H[3, 3] = np.nan
    with pytest.raises(qfa.QuflowHipError, match="QF_ERR_NONFINITE"):
        linalg.eigh(H)
    H[3, 3] = np.inf
    with pytest.raises(qfa.QuflowHipError, match="QF_ERR_NONFINITE"):
        linalg.eigvalsh(H)
    with pytest.raises(NotImplementedError, match="skew-Hermitian"):
        qfa.scale_decomposition(skew(16, 1), P=hermitian(16, False))
    # the context is as good as before
    G = hermitian(16, True)
    lam, V = linalg.eigh(G)
    check_decomposition(G, lam, V, "after the errors")
