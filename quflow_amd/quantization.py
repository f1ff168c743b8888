"""Spherical-harmonics <-> matrix transforms of quflow on the MI355X.

Mirrors `quflow.quantization` (quflow/quantization.py): `shr2mat`, `mat2shr`, `shc2mat`,
`mat2shc`, `get_basis`, `compute_basis`, `basis_break_index`, `elmr2mat`, `elmc2mat` with the reference's names,
argument meaning and conventions, so that initial data (`shr2mat(omega, N)`) and every
'shr' output of a run (`mat2shr(W)`, quflow/simulation.py:287-344) come from the device.

What runs where
  * the transforms -- one dense real (N-m)x(N-m) block of the basis times the m-th diagonal for
    every m -- are hand-written HIP kernels behind the C ABI (qf_shr2mat / qf_mat2shr /
    qf_shc2mat / qf_mat2shc), on one of two paths:
      - resident: the basis is uploaded once per context and stays in HBM (2.9 GB at N=1024,
        23 GB at N=2048); a transform is an HBM-bound sweep over it;
      - streamed (qf_basis_stream): no basis is stored.  Each call rebuilds the blocks it needs --
        m < Nmax, columns j < Nmax - m -- into a slab of bounded size and applies them there,
        slab after slab, with the same bits as the resident path.  Memory stays near N^2, so
        N = 4096 and 8192 (183 GB and 1.5 TB of basis) transform, and a band-limited call
        (n_omega = (lmax+1)^2) only builds about N Nmax^2 / 2 entries.
    `streamed=None` (the default of every transform) picks the resident path when a basis for N
    is already cached (`set_basis`, an earlier `get_basis`) or when it takes at most
    QUFLOW_HIP_BASIS_RESIDENT_MB (32768) MiB -- every N <= 2048 -- and streams otherwise, in slabs of
    QUFLOW_HIP_BASIS_SLAB_MB (4096) MiB; `streamed=True` / `False` force a path;
  * the basis itself (quantization.py:68-113: the eigenvectors of the tridiagonal blocks of the
    direct Laplacian, which the reference gets from LAPACK) is computed on the device as well
    (qf_basis_compute: the spectrum -el(el+1) is known, so each eigenvector is one twisted
    factorisation); `set_basis` installs a basis loaded from a reference-written file instead,
    which then takes the resident path.

There is no CPU path for the transforms: without the library or a GPU they raise.
"""
import ctypes
import os
import warnings

import numpy as np

from . import _lib
from .context import get_context, ptr

_basis_cache = dict()
_uploaded = dict()   # (device, N) -> id of the basis array resident on that context


# ---------------------
# LOWER LEVEL FUNCTIONS
# ---------------------

def elm2ind(el, m):
    """quflow/utils.py:91-105."""
    return el * el + el + m


def ind2elm(ind):
    """quflow/utils.py:73-89."""
    el = np.floor(np.sqrt(ind)).astype(int)
    m = ind - el * (el + 1)
    return el, m


def berezin_multipliers(N, dtype=np.float64, el=None):
    """w_l = sqrt(prod_{j<=l} (N-j)/(N+j)): Hoppe-Yau quantization T_N -> Berezin-Toeplitz Q_N,
    quflow/utils.py:108-135 (through log-gamma, as the reference)."""
    from math import lgamma
    if el is None:
        ells, _ = ind2elm(np.arange(N ** 2))
        ells = ells.astype(np.float64)
    else:
        ells = np.asarray(el, dtype=np.float64)
    NN = np.float64(N)
    lg = np.vectorize(lgamma, otypes=[np.float64])
    log_bw = 0.5 * (lgamma(NN + 1) + lgamma(NN) - lg(NN - ells) - lg(NN + ells + 1))
    return np.exp(log_bw).astype(dtype)


def basis_break_index(absm, N):
    """Start of the |m| block in the flat basis, quflow/quantization.py:24-42 (int or array)."""
    absm = np.asarray(absm, dtype=np.int64) - 1
    ind = absm + 2 * absm ** 2 - 6 * absm * N + 6 * N ** 2
    ind = ind * (1 + absm)
    out = ind // 6
    return int(out) if out.ndim == 0 else out


def basis_size(N):
    """sum_{m<N} (N-m)^2 = basis_break_index(N, N)."""
    return N * (N + 1) * (2 * N + 1) // 6


def compute_basis(N, dtype=np.float64, device=None):
    """Quantization basis, quflow/quantization.py:68-113, computed ON THE DEVICE (qf_basis_compute:
    one twisted factorisation per eigenvector at the known eigenvalues -el(el+1), where the
    reference calls LAPACK's tridiagonal eigensolver; same scaling sqrt(N), same orientation rule
    quantization.py:45-65) and returned as the reference's flat host array.  The copy in HBM stays
    resident for the transforms."""
    ctx = get_context(N, device)
    _lib.check(ctx._lib.qf_basis_compute(ctx.handle))
    basis = np.zeros(basis_size(N), dtype=np.float64)
    _lib.check(ctx._lib.qf_basis_download(ctx.handle, ptr(basis), ctypes.c_longlong(basis.shape[0])))
    if np.dtype(dtype) != np.float64:
        return basis.astype(dtype)
    _uploaded[(ctx.device, N)] = (id(basis), id(ctx))      # this very array is what sits in HBM
    return basis


# ----------------------
# HIGHER LEVEL FUNCTIONS
# ----------------------

def get_basis(N, allow_compute=True, dtype=np.double):
    """quflow/quantization.py:402-447 (memory cache, then computation; the reference's on-disk
    HDF5 cache is out of scope -- quflow/io.py)."""
    if isinstance(allow_compute, (type, np.dtype)):
        # the reference's own call sites pass the dtype in this slot (quantization.py:475)
        allow_compute = True
    key = (N, np.dtype(np.float64))
    if key in _basis_cache:
        return _basis_cache[key]
    basis = compute_basis(N) if allow_compute else None
    if basis is not None:
        _basis_cache[key] = basis
    return basis


def _basis_column(el, absm, N):
    """Column el - |m| of the |m| block of the basis: the |m|-th diagonal of T_{el,|m|}, N - |m| real numbers."""
    if not 0 <= absm <= el < N:
        raise ValueError("need 0 <= |m| <= el < N, got el=%d, m=%d, N=%d" % (el, absm, N))
    basis = get_basis(N)
    n = N - absm
    block = basis[basis_break_index(absm, N):basis_break_index(absm + 1, N)].reshape((n, n))
    return block[:, el - absm]


def elmr2mat(el, m, N, dtype=np.cdouble):
    """The real basis element T_{el,m} of u(N) as a scipy `dia_matrix` with the attribute `.el`
    (quflow/quantization.py:586-634), unit norm_L2.  The basis comes from the device (`get_basis`)."""
    from scipy.sparse import dia_matrix
    absm = abs(int(m))
    cdtype = np.complex64 if np.dtype(dtype) in (np.dtype(np.complex64), np.dtype(np.float32)) else np.complex128
    col = _basis_column(int(el), absm, N).astype(cdtype)
    if m == 0:
        T = dia_matrix((1.0j * col, 0), shape=(N, N))
    else:
        sgn = -1.0 if absm % 2 else 1.0
        d = col * ((sgn if m < 0 else 1.0j * sgn) / np.sqrt(2))
        data = np.zeros((2, N), dtype=cdtype)
        data[0, :N - absm] = -d.conj()
        data[1, absm:] = d
        T = dia_matrix((data, np.array([-absm, absm])), shape=(N, N))
    T.el = el
    return T


def elmc2mat(el, m, N, dtype=np.cdouble):
    """The complex basis element T_{el,m} of gl(N, C) as a scipy `dia_matrix` with the attribute `.el`
    (quflow/quantization.py:637-678), unit norm_L2."""
    from scipy.sparse import dia_matrix
    m = int(m)
    absm = abs(m)
    cdtype = np.complex64 if np.dtype(dtype) in (np.dtype(np.complex64), np.dtype(np.float32)) else np.complex128
    col = _basis_column(int(el), absm, N)
    data = np.zeros(N, dtype=cdtype)
    if m >= 0:
        data[:N - absm] = col
    else:
        data[absm:] = col
    data *= 1.0j if (m >= 0 or m % 2 == 0) else -1.0j
    T = dia_matrix((data, -m), shape=(N, N))
    T.el = el
    return T


def set_basis(N, basis):
    """Install a precomputed basis (e.g. one loaded from a reference-written file)."""
    basis = np.ascontiguousarray(basis, dtype=np.float64)
    if basis.shape != (basis_size(N),):
        raise ValueError("basis for N=%d must have %d entries, got %s" % (N, basis_size(N), basis.shape))
    _basis_cache[(N, np.dtype(np.float64))] = basis
    return basis


RESIDENT_MB = 32768     # QUFLOW_HIP_BASIS_RESIDENT_MB: the largest basis the automatic choice keeps resident
SLAB_MB = 4096          # QUFLOW_HIP_BASIS_SLAB_MB: the slab budget of the streamed path


def slab_bytes():
    """The streamed path's slab budget in bytes (QUFLOW_HIP_BASIS_SLAB_MB MiB)."""
    return int(float(os.environ.get("QUFLOW_HIP_BASIS_SLAB_MB", SLAB_MB)) * (1 << 20))


def use_streamed(N, streamed=None):
    """Whether a transform of size N streams the basis.  True / False force the path.  None: resident when a
    basis for N is cached (`set_basis`, an earlier `get_basis`: that very basis is what the transforms use) or
    when the basis takes at most QUFLOW_HIP_BASIS_RESIDENT_MB MiB; streamed otherwise."""
    if streamed is not None:
        return bool(streamed)
    if (N, np.dtype(np.float64)) in _basis_cache:
        return False
    limit = float(os.environ.get("QUFLOW_HIP_BASIS_RESIDENT_MB", RESIDENT_MB)) * (1 << 20)
    return basis_size(N) * 8 > limit


def _resident_context(N, device=None):
    """The context for N with the basis resident in HBM (uploaded once), in resident mode."""
    ctx = get_context(N, device)
    basis = get_basis(N)
    key = (ctx.device, N)
    if _uploaded.get(key) != (id(basis), id(ctx)):
        _lib.check(ctx._lib.qf_basis_upload(ctx.handle, ptr(basis), ctypes.c_longlong(basis.shape[0])))
        _uploaded[key] = (id(basis), id(ctx))
    _lib.check(ctx._lib.qf_basis_stream(ctx.handle, ctypes.c_longlong(0)))
    return ctx


def _transform_context(N, device=None, streamed=None):
    """The context for N with its mode set for this call (use_streamed)."""
    if not use_streamed(N, streamed):
        return _resident_context(N, device)
    ctx = get_context(N, device)
    _lib.check(ctx._lib.qf_basis_stream(ctx.handle, ctypes.c_longlong(slab_bytes())))
    return ctx


def shr2mat(omega, N=-1, berezin=False, device=None, *, streamed=None):
    """Real spherical harmonics -> matrix, quflow/quantization.py:450-489."""
    omega = np.asarray(omega)
    assert np.isrealobj(omega), "omega must be a real array."
    if N == -1:
        N = round(np.sqrt(omega.shape[0]))
    if berezin:      # quantization.py:475-481
        warnings.warn("Berezin scaling in shr2mat is ill adviced (it doesn't preserve energy or enstrophy)")
        bw = berezin_multipliers(N, omega.dtype)
        ind = np.nonzero(omega)
        omega = omega.copy()
        omega[ind] /= bw[ind]
    out_dtype = np.complex64 if omega.dtype == np.float32 else np.complex128
    om = np.ascontiguousarray(omega, dtype=np.float64)
    ctx = _transform_context(N, device, streamed)
    W_out = np.zeros((N, N), dtype=np.complex128)
    _lib.check(ctx._lib.qf_shr2mat(ctx.handle, ptr(om), ctypes.c_longlong(om.shape[0]), ptr(W_out)))
    return W_out.astype(out_dtype, copy=False)


def mat2shr(W, elmax=-1, berezin=False, device=None, *, streamed=None):
    """Matrix -> real spherical harmonics, quflow/quantization.py:492-525 (including its
    `elmax` convention: the output has ((elmax+1)^2)^2 entries)."""
    W = np.asarray(W)
    assert np.iscomplexobj(W), "W must be a complex array."
    N = W.shape[-1]
    Nmax = N
    if elmax > 0:
        Nmax = (elmax + 1) ** 2
    out_dtype = np.float32 if W.dtype == np.complex64 else np.float64
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    omega = np.zeros(Nmax ** 2, dtype=np.float64)
    ctx = _transform_context(N, device, streamed)
    _lib.check(ctx._lib.qf_mat2shr(ctx.handle, ptr(Wc), ptr(omega), ctypes.c_longlong(omega.shape[0])))
    if berezin:      # quantization.py:514-517
        warnings.warn("Berezin scaling in mat2shr is ill adviced. Use in shr2fun instead (default).")
        omega *= berezin_multipliers(N, omega.dtype)[:omega.shape[0]]
    return omega.astype(out_dtype, copy=False)


def shc2mat(omega, N=-1, berezin=False, device=None, *, streamed=None):
    """Complex spherical harmonics -> matrix, quflow/quantization.py:528-566."""
    omega = np.asarray(omega)
    if N == -1:
        N = round(np.sqrt(omega.shape[0]))
    else:
        if omega.shape[0] < N ** 2:
            omega = np.hstack((omega, np.zeros(N ** 2 - omega.shape[0])))
        else:
            omega = omega[:N ** 2]
    if berezin:      # quantization.py:548-553
        warnings.warn("Berezin scaling in shc2mat is ill adviced (it doesn't preserve energy or enstrophy)")
        bw = berezin_multipliers(N, np.float64)
        ind = np.nonzero(omega)
        omega = np.array(omega, dtype=np.complex128)
        omega[ind] /= bw[ind]
    om = np.ascontiguousarray(omega, dtype=np.complex128)
    ctx = _transform_context(N, device, streamed)
    W_out = np.zeros((N, N), dtype=np.complex128)
    _lib.check(ctx._lib.qf_shc2mat(ctx.handle, ptr(om), ptr(W_out)))
    return W_out


def mat2shc(W, berezin=False, device=None, *, streamed=None):
    """Matrix -> complex spherical harmonics, quflow/quantization.py:569-592."""
    W = np.asarray(W)
    N = W.shape[0]
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    omega = np.zeros(N ** 2, dtype=np.complex128)
    ctx = _transform_context(N, device, streamed)
    _lib.check(ctx._lib.qf_mat2shc(ctx.handle, ptr(Wc), ptr(omega)))
    if berezin:      # quantization.py:578-581
        warnings.warn("Berezin scaling in mat2shc is ill adviced. Use in shc2fun instead (default).")
        omega *= berezin_multipliers(N, np.float64)[:omega.shape[0]]
    return omega
