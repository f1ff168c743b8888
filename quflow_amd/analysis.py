"""Scale separation, spectra and random initial data: quflow.analysis on top of the device kernels.

Mirrors quflow/analysis.py: `scale_decomposition` (:8-34) and `energy_spectrum`, `enstrophy_spectrum`, `random_shr`,
`gamma_ratio` (:37-148), with the reference's names, arguments and operations (its loops over degrees vectorised).

For the spectra the data goes to real coefficients through `quflow_amd.sht.as_shr` -- a matrix through mat2shr, a function
or an image through the device analysis fun2shr -- and the sums over each degree are host numpy.

`scale_decomposition` runs on the device from end to end (qf_scale_decomposition): the eigenvectors V of the stream matrix
by the Hermitian eigensolver of `quflow_amd.linalg` applied to -i P, then Ws = V diag(diag(V^H W V)) V^H and Wr = W - Ws.
The reference calls the general `np.linalg.eig`; this package has a Hermitian solver only, which covers every stream
matrix of a skew-Hermitian state: a P that is not skew-Hermitian is refused (NotImplementedError), never sent to a CPU.
"""
import ctypes

import numpy as np

from . import _lib
from . import laplacian as _laplacian
from .laplacian import solve_poisson
from .quantization import mat2shr, ind2elm
from .sht import as_shr


def scale_decomposition(W, P=None, hamiltonian=solve_poisson):
    """(Ws, Wr): the canonical scale separation of the vorticity matrix W (quflow/analysis.py:8-34).  Ws is the part of W
    that commutes with the stream matrix P -- W in P's eigenbasis with the off-diagonal dropped -- and Wr = W - Ws.

    P is computed when not given: the built-in `solve_poisson` (ours, a PoissonHIP or the reference's) on the device
    inside the same call, any other `hamiltonian` by calling it on the host.  P must be skew-Hermitian."""
    from .context import as_c128, get_context, ptr
    from .integrators import _is_native_hamiltonian
    Wa = np.asarray(W)
    if Wa.dtype == np.complex64:
        raise NotImplementedError("scale_decomposition of a complex64 W: the eigensolver is double only; convert to "
                                  "complex128")
    Wc = as_c128(Wa, "W")
    N = Wc.shape[0]
    if P is None and not (_is_native_hamiltonian(hamiltonian) and _laplacian._SKEW_HERM_):
        # (the device's own solve is the skew-Hermitian form; after select_skewherm(False) the general one is asked for)
        P = (solve_poisson if hamiltonian is None else hamiltonian)(W)
    Pc = None
    if P is not None:
        Pc = as_c128(P, "P")
        if Pc.shape != Wc.shape:
            raise ValueError("W and P differ in shape: %s and %s" % (Wc.shape, Pc.shape))
        defect = np.abs(Pc + Pc.conj().T)
        if np.any(defect > N * np.finfo(np.float64).eps * np.abs(Pc).max()):
            raise NotImplementedError("scale_decomposition needs a skew-Hermitian stream matrix P (max|P + P^H| = %.3g): "
                                      "this package has a Hermitian eigensolver only, no general one and no CPU fallback"
                                      % defect.max())
    if N == 1:          # (no context that small; every 1 x 1 matrix commutes with P)
        return Wc.copy(), np.zeros_like(Wc)
    Ws = np.empty_like(Wc)
    Wr = np.empty_like(Wc)
    ctx = get_context(N)
    _lib.check_eigh(ctx._lib.qf_scale_decomposition(ctx.handle, ptr(Wc), ptr(Pc) if Pc is not None else None,
                                                    ptr(Ws), ptr(Wr)))
    return Ws, Wr


def _degree_sums(omegar):
    """N and sum_{|m| <= l} omegar[l, m]^2 for l = 1..N-1, each degree summed as numpy sums a slice."""
    N = round(np.sqrt(omegar.shape[0]))
    sq = np.asarray(omegar) ** 2
    return N, np.array([sq[el * el:(el + 1) * (el + 1)].sum() for el in range(1, N)], dtype=float).reshape(N - 1)


def energy_spectrum(data, beta=0):
    """(el, energy) for `data` as mat, omegar, omegac, fun or img: energy[el-1] = sum_m omega_lm^2 / (el (el+1))^(1-beta/2)
    (quflow/analysis.py:37-55)."""
    N, sums = _degree_sums(as_shr(data))
    el = np.arange(1, N)
    return el, sums / (el * (el + 1)) ** (1 - beta / 2)


def enstrophy_spectrum(data):
    """(el, enstrophy) with enstrophy[el-1] = sum_m omega_lm^2 (quflow/analysis.py:58-75)."""
    N, sums = _degree_sums(as_shr(data))
    return np.arange(1, N), sums


def _degrees(n):
    """The degree l of every index below n."""
    return ind2elm(np.arange(n))[0]


def random_shr(lmax=127, s=1.0, gamma=0.0, seed=None):
    """Random real coefficients up to degree lmax with Euclidean norm 1, as quflow.analysis.random_shr draws them (same
    stream of numpy's global generator, same arithmetic: bit-identical for the same arguments).

    Standard normal draws, the mean (index 0) removed, degree l damped by (l (l+1))^(s/2) (H^s smoothness).  `gamma` fixes
    |angular momentum| / sqrt(enstrophy), the l = 1 coefficients against all of l >= 1: 0 clears them, a value in (0, 1)
    rescales them, None leaves them as drawn."""
    count = (lmax + 1) ** 2
    if seed is not None:
        np.random.seed(seed)
    coeffs = np.random.randn(count)
    coeffs[0] = 0.0
    if s != 0.0:
        deg = _degrees(count)[1:]
        coeffs[1:] = coeffs[1:] / np.power(deg * (deg + 1), s / 2)
    momentum = coeffs[1:4]                       # a view: the three l = 1 coefficients
    if gamma == 0.0:
        momentum[:] = 0.0
    elif gamma is not None:
        # |momentum|^2 / (|momentum|^2 + rest) = gamma^2 with rest the enstrophy of l >= 2
        rest = np.sum(np.square(coeffs[4:]))
        target = np.sqrt(rest / (1 - gamma ** 2)) * gamma
        momentum *= target / np.linalg.norm(momentum)
    return coeffs / np.linalg.norm(coeffs)


def gamma_ratio(data):
    """|angular momentum| / sqrt(enstrophy): the norm of the l = 1 coefficients over the norm of all of them, for a
    matrix (through mat2shr) or a 1-D array of real coefficients (quflow.analysis.gamma_ratio)."""
    data = np.asarray(data)
    if data.ndim not in (1, 2):
        raise ValueError("gamma_ratio takes a matrix or a 1-D coefficient array, not %d dimensions" % data.ndim)
    coeffs = mat2shr(data) if data.ndim == 2 else data
    return np.linalg.norm(coeffs[1:4]) / np.linalg.norm(coeffs)
