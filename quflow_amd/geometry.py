"""Geometry helpers of quflow next to the hot path (quflow/geometry.py): `hbar` and the matrix
norms / inner products the diagnostics are made of on the host (O(N^2) reductions of a state that
is already there), `bracket` with its two products on the device, and the so(3) action on u(N):
`so3_generators` / `cartesian_generators` (host, O(N) numbers), `rotate`, `rotation_matrix` and `grad`
on the device (csrc/geometry.hip: the generators are tridiagonal with closed-form entries, so the
matrix exponential is one banded Taylor kernel and about log2(N |xi|) squarings, and the gradient is
one stencil pass -- DESIGN.md 8h).  Double precision, no CPU path."""
import numpy as np


def hbar(N):
    """hbar(N) = 2/sqrt(N^2-1)  (quflow/geometry.py:7-9)."""
    return 2.0 / np.sqrt(N ** 2 - 1)


def qtime2seconds(qtime, N):
    """Quantum time units -> seconds: qtime * hbar(N)  (quflow/utils.py:206-221)."""
    return qtime * (2.0 / np.sqrt(N ** 2 - 1))


def seconds2qtime(t, N):
    """Seconds -> quantum time units: t / hbar(N)  (quflow/utils.py:224-239)."""
    return t / (2.0 / np.sqrt(N ** 2 - 1))


def _device_matmul(A, B):
    from . import _lib
    from .context import as_c128, get_context, ptr, result_array
    A = as_c128(A, "A")
    B = as_c128(B, "B")
    C = result_array(A.shape, A.dtype, "matmul")
    ctx = get_context(A.shape[-1])
    _lib.check(ctx._lib.qf_zgemm(ctx.handle, ptr(A), ptr(B), ptr(C)))
    return C


def bracket(P, W):
    """[P, W]/hbar (quflow/geometry.py:41-49, dense branch), both products on the device."""
    A = _device_matmul(P, W)
    A -= _device_matmul(W, P)
    A /= hbar(np.asarray(P).shape[-1])
    return A


def norm_L2(W):
    """Scaled Frobenius norm (quflow/geometry.py:53-68)."""
    W = np.asarray(W)
    return np.linalg.norm(W, ord='fro') / np.sqrt(W.shape[-1])


def inner_L2(P, W):
    """Re sum P conj(W) / N (quflow/geometry.py:72-76)."""
    P = np.asarray(P)
    W = np.asarray(W)
    return (P * W.conj()).sum().real / W.shape[-1]


def norm_Linf(W):
    """Spectral norm (quflow/geometry.py:80-92)."""
    return np.linalg.norm(np.asarray(W), ord=2)


def norm_L1(W):
    """Scaled nuclear norm through the eigenvalues (quflow/geometry.py:95-110)."""
    W = np.asarray(W)
    sW = np.abs(np.linalg.eigvals(W))
    sW /= W.shape[-1]
    return sW.sum()


def integral(W):
    """Re(-i tr(W)/N) (quflow/geometry.py:113-129)."""
    W = np.asarray(W)
    trW = np.trace(W) / W.shape[-1]
    return np.real(-1j * trW)


def so3_generators(N, dtype=np.complex128):
    """(S1, S2, S3): the basis of the representation of so(3) in u(N) (quflow/geometry.py:132-151) as dense host arrays.
    With s = (N-1)/2 and c_a = sqrt((a+1)(N-1-a)): S3 = i diag(a - s), S1[a,a+1] = S1[a+1,a] = i c_a / 2,
    S2[a,a+1] = c_a / 2 = -S2[a+1,a]."""
    a = np.arange(N - 1, dtype=np.float64)
    half_c = np.sqrt((a + 1.0) * (N - 1.0 - a)) / 2
    S1 = 1j * (np.diag(half_c, 1) + np.diag(half_c, -1))
    S2 = (np.diag(half_c, 1) - np.diag(half_c, -1)).astype(np.complex128)
    S3 = 1j * np.diag(np.arange(N, dtype=np.float64) - (N - 1) / 2)
    return S1.astype(dtype), S2.astype(dtype), S3.astype(dtype)


def cartesian_generators(N, dtype=np.complex128):
    """(X1, X2, X3) = hbar(N) * (S1, S2, S3): the matrices of the Cartesian coordinate functions
    (quflow/geometry.py:173-194)."""
    h = hbar(N)
    S1, S2, S3 = so3_generators(N, dtype=dtype)
    return h * S1, h * S2, h * S3


def _rotation_vector(xi):
    xi = np.ascontiguousarray(xi, dtype=np.float64)
    if xi.shape != (3,):
        raise ValueError("xi must have shape (3,), got %s" % (xi.shape,))
    return xi


def _square(A, name):
    """(C-contiguous complex128 copy, dtype of the result): complex64 in -> computed in double -> complex64 out."""
    A = np.asarray(A)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 2:
        raise ValueError("%s must be a square matrix of size >= 2, got shape %s" % (name, A.shape))
    out_dtype = np.complex64 if A.dtype in (np.complex64, np.float32) else np.complex128
    return np.ascontiguousarray(A, dtype=np.complex128), out_dtype


def _xi_ptr(xi):
    import ctypes
    return xi.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def exp_plan(xi, N):
    """(squarings, degree) of the scaling rule for exp(xi . S) at size N (qf_so3_exp_plan; host only, no device):
    sigma = max(0, ceil(log2(|xi . S|_inf / 0.5))) and the smallest Taylor degree d with b^d / d! < 1e-18 for
    b = |xi . S|_inf / 2^sigma <= 0.5."""
    import ctypes
    from . import _lib
    xi = _rotation_vector(xi)
    sq, deg = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check_eigh(_lib.load().qf_so3_exp_plan(int(N), _xi_ptr(xi), ctypes.byref(sq), ctypes.byref(deg)))
    return sq.value, deg.value


def rotation_matrix(xi, N, device=None):
    """R = expm(xi[0] S1 + xi[1] S2 + xi[2] S3), (N,N) complex128 -- what the reference's `rotate` forms inline with
    scipy (quflow/geometry.py:168-169) -- on the device.  |xi| is not reduced modulo 2 pi.  Entrywise error a few
    N max(1, |xi|) eps."""
    from . import _lib
    from .context import get_context, ptr
    xi = _rotation_vector(xi)
    N = int(N)
    if N < 2:
        raise ValueError("N must be at least 2, got %d" % N)
    ctx = get_context(N, device)
    R = np.empty((N, N), dtype=np.complex128)
    _lib.check_eigh(ctx._lib.qf_so3_exp(ctx.handle, _xi_ptr(xi), ptr(R)))
    return R


def rotate(xi, W, device=None):
    """Axis-angle rotation of a vorticity matrix, R W R^H with R = rotation_matrix(xi, N) (quflow/geometry.py:154-170),
    for any complex W.  A NEW array.  complex64 input is computed in double and returned as complex64 (the reference
    would have computed in single there, so this result is the more accurate one)."""
    from . import _lib
    from .context import get_context, ptr
    xi = _rotation_vector(xi)
    Wc, out_dtype = _square(W, "W")
    ctx = get_context(Wc.shape[0], device)
    out = np.empty_like(Wc)
    _lib.check_eigh(ctx._lib.qf_rotate(ctx.handle, _xi_ptr(xi), ptr(Wc), ptr(out)))
    return out.astype(out_dtype, copy=False)


def grad(P, device=None):
    """(3,N,N): the matrices of the Cartesian gradient of P, dP[k] = bracket(X_k, P) = [S_k, P]
    (quflow/geometry.py:197-207), as one stencil pass on the device instead of six dense products.  A NEW array.
    complex64 input is computed in double and returned as complex64."""
    from . import _lib
    from .context import get_context, ptr
    Pc, out_dtype = _square(P, "P")
    N = Pc.shape[0]
    ctx = get_context(N, device)
    dP = np.empty((3, N, N), dtype=np.complex128)
    _lib.check_eigh(ctx._lib.qf_grad(ctx.handle, ptr(Pc), ptr(dP)))
    return dP.astype(out_dtype, copy=False)
