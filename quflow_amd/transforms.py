"""Spherical harmonics -> functions on the sphere, quflow.transforms on the MI355X.

Mirrors `quflow.transforms` (quflow/transforms.py) with the reference's names and argument rules:

  * `shr2fun`, `shc2fun` -- synthesis onto the MW grid (L, 2L-1) at bandwidth L: hand-written HIP kernels behind the C ABI
    (qf_shr2fun / qf_shc2fun, quflow_amd/csrc/sht.hip), where the reference calls pyssht or ducc0 (neither is needed here);
  * `state_fields` -- the function-space output rows of a state ('fun', 'funL2', 'funhalf', 'funL2half' of
    quflow/simulation.py:313-342) from one sweep of the basis and one stacked synthesis per bandwidth (qf_state_fields);
  * `as_fun`, `as_shr` -- the reference's dispatch on the kind of data;
  * `shr2shc`, `shc2shr`, `sphgrid`, `fun2img`, `img2fun` -- host numpy, as in the reference (vectorised).

The analysis direction `fun2shc` / `fun2shr` (and `as_shr` of a function or an image) lives in `quflow_amd.sht`; the
three names here still raise NotImplementedError.  There is no CPU path for the synthesis: without the library or a GPU
it raises.
"""
import ctypes
from math import isqrt

import numpy as np

from . import _lib
from .context import get_context, ptr
from .quantization import mat2shr, mat2shc, ind2elm

LMAX = 8192      # the largest bandwidth the synthesis kernels take


def sphgrid(N):
    """MW sampling at bandwidth N (quflow/utils.py:179-203): theta_t = pi (2t+1)/(2N-1), phi_p = 2 pi p/(2N-1), returned
    as two (N, 2N-1) arrays (theta along the rows)."""
    theta = (2.0 * np.arange(N) + 1.0) * np.pi / (2.0 * N - 1.0)
    phi = 2.0 * np.arange(2 * N - 1) * np.pi / (2.0 * N - 1.0)
    phig, thetag = np.meshgrid(phi, theta)
    return thetag, phig


def _full_degrees(n):
    """Degrees el < E that shr2shc / shc2shr convert for an array of n entries.  The reference walks el while its m = 0
    entry el^2 + el lies in the array and indexes all of -el..el: a last degree cut short raises IndexError there, and so
    it does here."""
    if n < 1:
        raise IndexError("index 0 is out of bounds for axis 0 with size %d" % n)
    el = isqrt(n - 1)
    while el * el + el >= n:
        el -= 1
    if el * el + 2 * el >= n:
        raise IndexError("index %d is out of bounds for axis 0 with size %d" % (el * el + 2 * el, n))
    return el + 1


def shr2shc(omega_real):
    """Real -> complex spherical harmonics, quflow/transforms.py:310-349 (vectorised, the same operations)."""
    omega_real = np.asarray(omega_real)
    n = omega_real.shape[0]
    E = _full_degrees(n)
    omega_complex = np.zeros(n, dtype=complex)
    el, m = ind2elm(np.arange(E * E))
    mid = el * el + el
    z, ng, ps = m == 0, m < 0, m > 0
    omega_complex[np.nonzero(z)[0]] = omega_real[mid[z]]
    omega_complex[np.nonzero(ng)[0]] = (1. / np.sqrt(2)) * (omega_real[mid[ng] - m[ng]] - 1j * omega_real[mid[ng] + m[ng]])
    sgn = np.where(m[ps] % 2 == 1, -1, 1)
    omega_complex[np.nonzero(ps)[0]] = (1. / np.sqrt(2)) * sgn * (omega_real[mid[ps] + m[ps]] + 1j * omega_real[mid[ps] - m[ps]])
    return omega_complex


def shc2shr(omega_complex):
    """Complex -> real spherical harmonics, quflow/transforms.py:271-307 (vectorised, the same operations); a projection
    when omega_complex is not the expansion of a real function."""
    omega_complex = np.asarray(omega_complex)
    n = omega_complex.shape[0]
    E = _full_degrees(n)
    omega_real = np.zeros(n, dtype=float)
    el, m = ind2elm(np.arange(E * E))
    mid = el * el + el
    z, ng, ps = m == 0, m < 0, m > 0
    omega_real[np.nonzero(z)[0]] = omega_complex[mid[z]].real
    omega_real[np.nonzero(ng)[0]] = np.sqrt(2) * (-1) ** (-m[ng]) * omega_complex[mid[ng] - m[ng]].imag
    omega_real[np.nonzero(ps)[0]] = np.sqrt(2) * (-1) ** m[ps] * omega_complex[mid[ps] + m[ps]].real
    return omega_real


def fun2img(f, lim=np.inf):
    """A 2D float array as an 8-bit image, quflow/transforms.py:352-380 (lim: (low, high) or a symmetric bound; by default
    max |f|, so that 0.0 maps to 127)."""
    if not isinstance(lim, tuple):
        if lim == np.inf:
            lim = np.abs(f).max()
        lim = (-lim, lim)
    return np.clip(255 * (f - lim[0]) / (lim[1] - lim[0]), 0, 255).astype(np.uint8)


def img2fun(img, lim=1.0):
    """An 8-bit image as a float array, quflow/transforms.py:383-401."""
    if not isinstance(lim, tuple):
        lim = (-lim, lim)
    return img.astype(float) * (lim[1] - lim[0]) / 255. + lim[0]


def fun2shc(f):
    """Not implemented: MW analysis (grid -> coefficients) is out of scope for quflow_amd."""
    raise NotImplementedError("fun2shc: the MW analysis (grid -> coefficients) is not implemented in quflow_amd; only the "
                              "synthesis shc2fun / shr2fun is")


def fun2shr(f):
    """Not implemented: MW analysis (grid -> coefficients) is out of scope for quflow_amd."""
    raise NotImplementedError("fun2shr: the MW analysis (grid -> coefficients) is not implemented in quflow_amd; only the "
                              "synthesis shc2fun / shr2fun is")


def _bandwidth(n, N):
    """L of the reference's shc2fun (transforms.py:245-256): inferred from a square length when N == -1, else N."""
    if N == -1:
        L = isqrt(n - 1) + 1 if n >= 1 else 0
        if n < 1 or L * L != n:
            raise AssertionError("It seems that omega does not have the right length (%d is not a square)." % n)
    else:
        L = int(N)
    if not 1 <= L <= LMAX:
        raise ValueError("bandwidth L=%d is outside 1..%d" % (L, LMAX))
    return L


def shc2fun(omega, isreal=False, N=-1, berezin=True, device=None):
    """Complex spherical harmonics -> MW grid (L, 2L-1), quflow/transforms.py:220-268, on the device.

    f = sqrt(4 pi) sum_{l<L, |m|<=l} w_l omega[l^2+l+m] Y_lm(theta_t, phi_p), Y_lm orthonormal with the Condon-Shortley
    phase, w_l = berezin_multipliers(L)[l] (the multipliers of the bandwidth, not of a matrix size) or 1.  L is inferred
    from a square len(omega) when N == -1; otherwise omega is trimmed or zero-padded to L^2 entries.  Returns complex128,
    or float64 when `isreal`: then only the m >= 0 coefficients enter, as in a real-map synthesis,
        f = sum_l Re(a_l0) lambda_l0 + 2 sum_{m>0} Re(a_lm lambda_lm e^{i m phi}).
    That Im(a_l0) takes no part is inferred from how a real synthesis works (ducc0's synthesis_2d of real maps reads only
    m >= 0); it has not been checked against ducc0 itself, which is not available here.

    The multipliers are formed on the host in long double as prod_{j<=l} (L-j)/(L+j), the product the reference's
    log-gamma expression stands for; the two agree to the reference's own rounding (a few 1e-13 relative at L = 512)."""
    omega = np.asarray(omega)
    L = _bandwidth(omega.shape[0], N)
    om = np.ascontiguousarray(omega[:L * L], dtype=np.complex128)
    if om.shape[0] == 0:
        om = np.zeros(1, dtype=np.complex128)
    f = np.empty((L, 2 * L - 1), dtype=np.float64 if isreal else np.complex128)
    ctx = get_context(max(L, 2), device)
    _lib.check(ctx._lib.qf_shc2fun(ctx.handle, ptr(om), ctypes.c_longlong(om.shape[0]), L, int(bool(berezin)),
                                   int(bool(isreal)), ptr(f)))
    return f


def shr2fun(omega, N=-1, berezin=True, device=None):
    """Real spherical harmonics -> MW grid (L, 2L-1), float64: shc2fun(shr2shc(omega), isreal=True, N) (quflow/
    transforms.py:422-438).  The conversion to complex coefficients happens on the device, with the same operations as
    shr2shc, so the two routes give the same bits."""
    omega = np.asarray(omega)
    assert np.isrealobj(omega), "omega must be a real array."
    _full_degrees(omega.shape[0])           # the reference's shr2shc raises for a cut-short last degree
    L = _bandwidth(omega.shape[0], N)
    om = np.ascontiguousarray(omega[:L * L], dtype=np.float64)
    f = np.empty((L, 2 * L - 1), dtype=np.float64)
    ctx = get_context(max(L, 2), device)
    _lib.check(ctx._lib.qf_shr2fun(ctx.handle, ptr(om), ctypes.c_longlong(om.shape[0]), L, int(bool(berezin)), ptr(f)))
    return f


# ---- function-space output of a state: the reference's 'fun' / 'funL2' / 'funhalf' / 'funL2half' qutypes
# (quflow/simulation.py:41, 313-342): the variable a row is stored under
FUNCTION_VARNAMES = {'fun': 'fun', 'funhalf': 'fun', 'funL2': 'funL2', 'funL2half': 'funL2'}


def field_spec(qutype, N):
    """(n_omega, berezin, variable name) of a function-space qutype for an N x N state: 'half' keeps the leading
    (N//2)**2 coefficients (simulation.py:336-337), 'L2' switches the Berezin multipliers off (:338-339)."""
    if qutype not in FUNCTION_VARNAMES:
        raise KeyError("'%s' is not a function-space qutype; available: %s" % (qutype, sorted(FUNCTION_VARNAMES)))
    n_omega = (N // 2) ** 2 if 'half' in qutype else N * N
    return n_omega, 'L2' not in qutype, FUNCTION_VARNAMES[qutype]


def check_function_qutypes(qutypes):
    """The function-space part of a qutypes dict as {qutype: numpy dtype}, checked: the reference's two ValueErrors for
    'fun' + 'funhalf' and 'funL2' + 'funL2half' (simulation.py:122-126, both rows would go to one variable), real dtypes
    float32 / float64 only (None: float64, what the reference's np.array(..., dtype=None) makes).  A complex dtype is
    refused: the reference's branch for it hands real coefficients to shc2fun, which is not mirrored."""
    if 'fun' in qutypes and 'funhalf' in qutypes:
        raise ValueError("Cannot have both fun and funhalf outputs.")
    if 'funL2' in qutypes and 'funL2half' in qutypes:
        raise ValueError("Cannot have both funL2 and funL2half outputs.")
    out = {}
    for q, dtype in qutypes.items():
        if q not in FUNCTION_VARNAMES:
            continue
        dt = np.dtype(np.float64 if dtype is None else dtype)
        if dt.kind == 'c':
            raise NotImplementedError("qutype '%s' with the complex dtype %s: complex function-space rows are not written "
                                      "(use float32 or float64)" % (q, dt))
        if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise NotImplementedError("qutype '%s' with dtype %s: function-space rows are float32 or float64" % (q, dt))
        out[q] = dt
    return out


def _fields_call(ctx, W, N, qutypes):
    """qf_state_fields on `ctx` for the state W (None: the resident state): {qutype: (L, 2L-1) array}."""
    qutypes = dict(qutypes)
    unknown = [q for q in qutypes if q not in FUNCTION_VARNAMES]
    if unknown:
        raise KeyError("not function-space qutypes: %s; available: %s" % (unknown, sorted(FUNCTION_VARNAMES)))
    dtypes = check_function_qutypes(qutypes)
    if not dtypes:
        return {}
    specs = (_lib.Field * len(dtypes))()
    outs, ptrs = {}, (ctypes.c_void_p * len(dtypes))()
    for i, (q, dt) in enumerate(dtypes.items()):
        n_omega, berezin, _ = field_spec(q, N)
        if n_omega < 1:
            raise ValueError("qutype '%s' keeps (N//2)**2 = 0 coefficients at N=%d" % (q, N))
        L = _bandwidth(n_omega, -1)
        specs[i] = _lib.Field(n_omega, int(berezin), 1 if dt == np.dtype(np.float32) else 0)
        outs[q] = np.empty((L, 2 * L - 1), dtype=dt)
        ptrs[i] = outs[q].ctypes.data
    _lib.check(ctx._lib.qf_state_fields(ctx.handle, None if W is None else ptr(W), len(dtypes), specs, ptrs))
    return outs


def state_fields(W, qutypes, device=None):
    """The function-space outputs of a state, {qutype: array}: for each of 'fun', 'funL2', 'funhalf', 'funL2half' in
    `qutypes` (a dict {qutype: float32 / float64}, the reference's form) the grid shr2fun(mat2shr(W)[:n], berezin=...) cast
    to its dtype, bit for bit, from ONE sweep of the basis and one stacked synthesis per bandwidth (qf_state_fields); the
    cast happens on the device, so a float32 grid crosses PCIe as float32.  W: an (N,N) complex matrix, or a (k,N,N) stack,
    whose fields come back as (k, L, 2L-1) arrays, member by member."""
    W = np.asarray(W)
    assert np.iscomplexobj(W), "W must be a complex array."
    N = W.shape[-1]
    if W.ndim == 3:
        rows = [state_fields(Wi, qutypes, device) for Wi in W]
        return {q: np.array([r[q] for r in rows]) for q in (rows[0] if rows else {})}
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    from .quantization import _transform_context
    return _fields_call(_transform_context(N, device), Wc, N, qutypes)


def as_fun(data, N=-1, **kwargs):
    """Take `fun`, `img`, `omegar`, `omegac` or `mat` data to `fun`, quflow/transforms.py:441-486: a skew-Hermitian matrix
    goes through mat2shr and shr2fun, any other square complex matrix through mat2shc and shc2fun (complex output), a
    float or uint8 image passes through (img2fun for the latter), and coefficient arrays go to the synthesis.
    (The reference hands N to shc2fun positionally, where it lands in `isreal`; here it is the bandwidth.)"""
    data = np.asarray(data)
    if data.ndim == 2:
        if data.shape[0] == data.shape[1] and np.iscomplexobj(data):
            W = data
            if N == -1:
                N = W.shape[0]
            if np.allclose(W, -W.conj().T):
                return shr2fun(mat2shr(W), N, **kwargs)
            return shc2fun(mat2shc(W), N=N, **kwargs)
        if data.dtype == np.uint8:
            return img2fun(data)
        return data
    if np.iscomplexobj(data):
        return shc2fun(data, N=N, **kwargs)
    return shr2fun(data, N, **kwargs)


def as_shr(data):
    """Take `img`, `omegar`, `omegac` or `mat` data to `omegar`, quflow/transforms.py:489-530.  A function or image would
    need the analysis fun2shr, which is not implemented: NotImplementedError."""
    data = np.asarray(data)
    if data.ndim == 2:
        if data.shape[0] == data.shape[1] and np.iscomplexobj(data):
            return mat2shr(data)
        return fun2shr(img2fun(data) if data.dtype == np.uint8 else data)
    if np.iscomplexobj(data):
        return shc2shr(data)
    return data
