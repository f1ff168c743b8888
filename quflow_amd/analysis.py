"""Spectra and random initial data, quflow.analysis on top of the device transforms.

Mirrors quflow/analysis.py:37-148: `energy_spectrum`, `enstrophy_spectrum`, `random_shr`, `gamma_ratio`, with the
reference's names, arguments and operations (its loops over degrees vectorised).  The data goes to real coefficients
through `quflow_amd.sht.as_shr` -- a matrix through mat2shr, a function or an image through the device analysis fun2shr --
and the sums over each degree are host numpy.

Not here: `scale_decomposition` (quflow/analysis.py:8-34) needs a dense non-Hermitian eigensolver, which this package
does not have.
"""
import numpy as np

from .quantization import mat2shr, ind2elm
from .sht import as_shr


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
