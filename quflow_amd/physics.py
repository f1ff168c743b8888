"""Diagnostics of the hot path (quflow/physics.py:26-38) evaluated on the device, and the Sobolev
inner products next to them (quflow/physics.py:9-21: one device solve / stencil, one host reduction)."""
import ctypes

import numpy as np

from . import _lib
from .context import as_c128, get_context, ptr


def _diagnostics(W):
    W = np.asarray(W)
    if W.ndim >= 3:
        W = W[(0,) * (W.ndim - 2) + (Ellipsis,)]
    Wc = as_c128(W, "W")
    ctx = get_context(Wc.shape[-1])
    _lib.check(ctx._lib.qf_upload_W(ctx.handle, ptr(Wc)))
    e = ctypes.c_double()
    s = ctypes.c_double()
    _lib.check(ctx._lib.qf_diagnostics(ctx.handle, ctypes.byref(e), ctypes.byref(s)))
    return e.value, s.value


def energy_euler(W):
    """E = -<W, Delta^-1 W>/2, quflow/physics.py:26-32."""
    return _diagnostics(W)[0]


def enstrophy(W):
    """S = <W, W>/2, quflow/physics.py:34-38."""
    return _diagnostics(W)[1]


CASIMIR_KMAX = 8


def check_kmax(kmax):
    """The highest Casimir asked for as an int in 1..8; ValueError otherwise (before anything touches a device)."""
    if isinstance(kmax, bool) or not isinstance(kmax, (int, np.integer)) or not 1 <= kmax <= CASIMIR_KMAX:
        raise ValueError("kmax must be an integer in 1..%d, got %r" % (CASIMIR_KMAX, kmax))
    return int(kmax)


def casimirs_call(fn, kmax, *args):
    """One of the qf_*casimirs entry points with its trailing (kmax, out) arguments: the (kmax,) ndarray.  An inf or NaN
    in the matrix raises ValueError (QF_ERR_NONFINITE)."""
    out = np.empty(kmax, dtype=np.float64)
    _lib.check(fn(*args, kmax, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return out


def casimirs(W, kmax=4):
    """The Casimirs C_k = Re tr((iW)^k) / N, k = 1..kmax <= 8, of a host matrix, formed on the device (qf_casimirs): an
    ndarray of shape (kmax,).  Any complex W -- nothing assumes skew-Hermitian symmetry; complex64 input is computed in
    complex128.  C_2 = <W, W> = 2 enstrophy(W).  What the isospectral steppers conserve; a `Simulation` logger as it
    stands.  A stack (..., N, N) is read at its first member, as energy_euler and enstrophy do."""
    kmax = check_kmax(kmax)
    W = np.asarray(W)
    if W.ndim >= 3:
        W = W[(0,) * (W.ndim - 2) + (Ellipsis,)]
    Wc = as_c128(W, "W")
    ctx = get_context(Wc.shape[-1])
    return casimirs_call(ctx._lib.qf_casimirs, kmax, ctx.handle, ptr(Wc))


def mhd_diagnostics(state):
    """The diagnostics of the MHD state (W, Theta), a (2,N,N) array, in one device call (qf_mhd_diagnostics: one Poisson
    solve, one reduction pass): a dict with energy_kinetic = -<W, Delta^-1 W>/2, energy_magnetic = -<Theta, Delta Theta>/2,
    energy = their sum (the conserved Hamiltonian of quflow/integrators/mhd.py's system), cross_helicity = <W, Theta>,
    magnetic_casimir = <Theta, Theta>/2 and enstrophy = <W, W>/2.  DeviceMHDTrajectory.diagnostics() of a resident state."""
    from .integrators import _mhd_dict
    state = np.asarray(state)
    if state.ndim != 3 or state.shape[0] != 2 or state.shape[1] != state.shape[2]:
        raise ValueError("the MHD state must be a (2,N,N) array (W, Theta), got shape %s" % (state.shape,))
    sc = np.ascontiguousarray(state, dtype=np.complex128)
    ctx = get_context(sc.shape[-1])
    _lib.check(ctx._lib.qf_states_upload(ctx.handle, ptr(sc), 2))
    d = (ctypes.c_double * 5)()
    _lib.check(ctx._lib.qf_mhd_diagnostics(ctx.handle, d))
    return _mhd_dict(d)


def energy_mhd(state):
    """H = -<W, Delta^-1 W>/2 - <Theta, Delta Theta>/2 of the MHD state (W, Theta)."""
    return mhd_diagnostics(state)["energy"]


def cross_helicity(state):
    """<W, Theta> of the MHD state (W, Theta)."""
    return mhd_diagnostics(state)["cross_helicity"]


def magnetic_energy(Theta):
    """-<Theta, Delta Theta>/2 for the magnetic potential Theta, an (N,N) matrix."""
    Theta = np.asarray(Theta)
    if Theta.ndim != 2 or Theta.shape[0] != Theta.shape[1]:
        raise ValueError("Theta must be a square matrix, got shape %s" % (Theta.shape,))
    return mhd_diagnostics(np.stack([Theta, Theta]))["energy_magnetic"]


def inner_Hm1(W1, W2):
    """-<W1, Delta^-1 W2>, quflow/physics.py:9-11."""
    from .geometry import inner_L2
    from .laplacian import solve_poisson
    return -inner_L2(W1, solve_poisson(W2))


def norm_Hm1(W):
    """quflow/physics.py:13-14."""
    return np.sqrt(inner_Hm1(W, W))


def inner_H1(P1, P2):
    """-<P1, Delta P2>, quflow/physics.py:16-18."""
    from .geometry import inner_L2
    from .laplacian import laplace
    return -inner_L2(P1, laplace(P2))


def norm_H1(P):
    """quflow/physics.py:20-21."""
    return np.sqrt(inner_H1(P, P))


def sectional_curvature(F, G):
    """The sectional curvature expression of quflow/physics.py:41-58 for the pair (F, G), composed of the device
    `laplace`, `solve_poisson`, `commutator` and the host `inner_L2` exactly as there."""
    from . import integrators
    from .geometry import inner_L2
    from .laplacian import laplace, solve_poisson
    commutator = integrators.commutator
    LF, LG = laplace(F), laplace(G)
    FG = commutator(F, G)
    LF_G = commutator(LF, G)
    LG_F = commutator(LG, F)
    LF_F = commutator(LF, F)
    LG_G = commutator(LG, G)
    sym = LF_G + LG_F
    C = -inner_L2(sym, solve_poisson(sym)) / 4.0
    C -= inner_L2(FG, LF_G - LG_F) / 2.0
    C += inner_L2(FG, laplace(FG)) * (3.0 / 4.0)
    C += inner_L2(LF_F, solve_poisson(LG_G))
    return C
