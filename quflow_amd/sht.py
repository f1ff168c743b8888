"""Functions on the sphere -> spherical harmonics: the analysis half of quflow.transforms on the MI355X.

`fun2shc`, `fun2shr` and `as_shr` with the reference's names and argument rules (quflow/transforms.py:189-217, 404-419,
489-530).  The transform is McEwen-Wiaux analysis on the grid of `transforms.sphgrid`, as pyssht (the reference's first
choice) defines it; for f of shape (L, P), P = 2L-1:

  1. ring DFT  F_m(t) = (1/P) sum_p f[t, p] e^{-2 pi i m p/P},  |m| < L;
  2. extension to the full circle, F_m(theta_{P-1-t}) = (-1)^m F_m(theta_t) for t < L-1 (the ring theta = pi is kept);
  3. the trigonometric interpolant of those P values, degrees |m'| < L;
  4. a_lm = 2 pi int_0^pi F_m(theta) lambda_lm(theta) sin(theta) d theta, exactly;
  5. fun2shc(f)[l^2 + l + m] = a_lm / sqrt(4 pi),  fun2shr(f) = shc2shr(fun2shc(f)).

For band-limited f this inverts `transforms.shc2fun(., berezin=False)`; for any other array it is the same fixed linear
map.  ducc0's MW analysis (the reference's second choice) may differ from it on arrays whose odd-m ring DFT does not vanish
on the ring theta = pi; that has not been checked, ducc0 is not available here.

Everything runs in hand-written HIP kernels behind qf_fun2shc / qf_fun2shr (quflow_amd/csrc/sht.hip);
there is no CPU path: without the library or a GPU the calls raise.

`quflow_amd.transforms.fun2shc`, `fun2shr` and `as_shr` (and their re-exports in the package) still refuse a function
or an image by name; pointing them here is a follow-up of a few lines, together with the test that pins the refusal.
"""
import numpy as np

from . import _lib
from .context import get_context, ptr
from .quantization import mat2shr
from .transforms import LMAX, shc2shr, img2fun


_CTX_N = 2     # the analysis does not depend on the context's N: every bandwidth runs on the one smallest context


def _context(device):
    """The context of the analysis entry points: one per device, whatever L, so that a sweep over bandwidths keeps one set
    of ctx->sht buffers and one pair of theta operators (rebuilt when L changes) instead of a solver context per L."""
    return get_context(_CTX_N, device)


def _grid(f):
    """The reference's input rules (transforms.py:205-211): (N, 2N-1), real or complex, cast to float / complex."""
    f = np.ascontiguousarray(f)
    assert f.ndim == 2 and 2 * f.shape[0] - 1 == f.shape[1], "Shape of input must be (N, 2*N-1)."
    isreal = not np.iscomplexobj(f)
    f = np.ascontiguousarray(f, dtype=np.float64 if isreal else np.complex128)
    L = f.shape[0]
    if not 1 <= L <= LMAX:
        raise ValueError("bandwidth L=%d is outside 1..%d" % (L, LMAX))
    return f, L, isreal


def fun2shc(f, device=None):
    """MW grid (N, 2N-1), real or complex -> N^2 complex spherical-harmonic coefficients (quflow/transforms.py:189-217),
    on the device.  A real grid gives a_l,-m = (-1)^m conj(a_lm)."""
    f, L, isreal = _grid(f)
    omega = np.empty(L * L, dtype=np.complex128)
    ctx = _context(device)
    _lib.check(ctx._lib.qf_fun2shc(ctx.handle, ptr(f), L, int(isreal), ptr(omega)))
    return omega


def fun2shr(f, device=None):
    """MW grid (N, 2N-1) -> N^2 real coefficients, shc2shr(fun2shc(f)) (quflow/transforms.py:404-419).  The conversion
    happens on the device with shc2shr's operations, so the two routes give the same bits."""
    f, L, isreal = _grid(f)
    omega = np.empty(L * L, dtype=np.float64)
    ctx = _context(device)
    _lib.check(ctx._lib.qf_fun2shr(ctx.handle, ptr(f), L, int(isreal), ptr(omega)))
    return omega


def as_shr(data, device=None):
    """Take `fun`, `img`, `omegar`, `omegac` or `mat` data to `omegar`, quflow/transforms.py:489-530, with the `fun` and
    `img` branches going through fun2shr."""
    data = np.asarray(data)
    if data.ndim == 2:
        if data.shape[0] == data.shape[1] and np.iscomplexobj(data):
            return mat2shr(data)
        return fun2shr(img2fun(data) if data.dtype == np.uint8 else data, device=device)
    if np.iscomplexobj(data):
        return shc2shr(data)
    return data
