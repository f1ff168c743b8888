"""Hermitian eigendecompositions on the device (csrc/eigh.hip behind qf_eigh / qf_eigh_skew).

    lam, V = eigh(H)             # H = V diag(lam) V^H, lam ascending, V unitary       (numpy.linalg.eigh)
    lam = eigvalsh(H)            # the same eigenvalues, bit for bit, without V          (numpy.linalg.eigvalsh)
    lam, V = eig_skewherm(W)     # W = V diag(i lam) V^H for a skew-Hermitian W: the decomposition of -i W

The solver is a parallel one-sided Jacobi iteration in double precision: complex128 only, no CPU path, and
two calls return the same bits.  The arguments are checked on the host before any device call: a square matrix,
Hermitian (skew-Hermitian) to N eps max|H|.  There is nothing to compute for a 1 x 1 matrix, and no context that small:
its eigenvalue is read off here.
"""
import ctypes

import numpy as np

from . import _lib
from .context import get_context, ptr

_EPS = np.finfo(np.float64).eps


def _checked(A, name, sign):
    """C-contiguous complex128 copy of a square matrix with A^H = sign * A to N eps max|A|."""
    A = np.asarray(A)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 1:
        raise ValueError("%s must be a square matrix, got shape %s" % (name, A.shape))
    if A.dtype == np.complex64 or A.dtype == np.float32:
        raise NotImplementedError("%s is %s: the eigensolver is double only; convert to complex128" % (name, A.dtype))
    A = np.ascontiguousarray(A, dtype=np.complex128)
    N = A.shape[0]
    # (an inf or NaN passes here and is reported by the device call, as QF_ERR_NONFINITE)
    with np.errstate(invalid="ignore"):
        defect = np.abs(A - sign * A.conj().T)
        scale = np.abs(A).max()
        bad = np.any(defect > N * _EPS * scale)
    if bad:
        raise ValueError("%s is not %sHermitian to N eps max|%s| (defect %.3g, max entry %.3g)"
                         % (name, "skew-" if sign < 0 else "", name, np.nanmax(defect), scale))
    return A


def _decompose(A, skew, vectors, device):
    N = A.shape[0]
    if N == 1:
        z = complex(A[0, 0])
        if not np.isfinite(z.real) or not np.isfinite(z.imag):
            raise _lib.QuflowHipError("QF_ERR_NONFINITE: eigh: the matrix has an inf or NaN entry")
        lam = np.array([z.imag if skew else z.real])
        return (lam, np.ones((1, 1), dtype=np.complex128)) if vectors else lam
    ctx = get_context(N, device)
    lam = np.empty(N, dtype=np.float64)
    V = np.empty((N, N), dtype=np.complex128) if vectors else None
    st = _lib.EighStats()
    fn = ctx._lib.qf_eigh_skew if skew else ctx._lib.qf_eigh
    _lib.check_eigh(fn(ctx.handle, ptr(A), ptr(lam), ptr(V) if vectors else None, ctypes.byref(st)))
    _decompose.last_stats = {"sweeps": st.sweeps, "rotations": st.rotations, "off": st.off}
    return (lam, V) if vectors else lam


_decompose.last_stats = None


def last_stats():
    """{"sweeps", "rotations", "off"} of the most recent decomposition of this process (None before the first)."""
    return _decompose.last_stats


def eigh(H, device=None):
    """(lam, V) with H = V diag(lam) V^H: lam ascending float64, V unitary complex128, column j belonging to lam[j]."""
    return _decompose(_checked(H, "H", 1.0), False, True, device)


def eigvalsh(H, device=None):
    """The ascending eigenvalues of the Hermitian matrix H: the bits of eigh(H)[0]."""
    return _decompose(_checked(H, "H", 1.0), False, False, device)


def eig_skewherm(W, device=None, vectors=True):
    """(lam, V) with W = V diag(1j * lam) V^H for a skew-Hermitian W (-i W is formed and decomposed on the device);
    lam alone with vectors=False."""
    return _decompose(_checked(W, "W", -1.0), True, bool(vectors), device)
