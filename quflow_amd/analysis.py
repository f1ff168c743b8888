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
from .context import ptr
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


def _band_limit(N, lmax):
    """The band limit Nmax (degrees l < Nmax) of a budget call: N, or `lmax` in (1, N]."""
    if lmax is None:
        return int(N)
    if isinstance(lmax, (bool, np.bool_)) or int(lmax) != lmax:
        raise ValueError("lmax must be an integer in (1, N], got %r" % (lmax,))
    if not 1 < int(lmax) <= N:
        raise ValueError("lmax must lie in (1, N] = (1, %d], got %d" % (N, int(lmax)))
    return int(lmax)


def _budget_dict(rows, has_forcing, strang_splitting=None, coeffs=None):
    """The budget's dictionary from the device's rows (3, Nmax) = Z_l, T_l, I_l, l = 0..Nmax-1: host arithmetic only.
    Everything is reported for el = 1..Nmax-1 (as the spectra of this module); an energy form divides the enstrophy
    quantity by el (el + 1), a flux is minus the running sum of its transfer, and the dissipation of a
    ViscDampStep(nu, alpha) is -2 (nu el (el+1) + alpha) Z_l."""
    rows = np.asarray(rows, dtype=np.float64)
    nmax = rows.shape[1]
    el = np.arange(1, nmax)
    ll = (el * (el + 1)).astype(np.float64)
    Z, T = rows[0, 1:].copy(), rows[1, 1:].copy()
    out = {"el": el, "enstrophy": Z, "energy": Z / ll,
           "enstrophy_transfer": T, "energy_transfer": T / ll}
    out["enstrophy_flux"] = -np.cumsum(out["enstrophy_transfer"])
    out["energy_flux"] = -np.cumsum(out["energy_transfer"])
    if has_forcing:
        out["enstrophy_input"] = rows[2, 1:].copy()
        out["energy_input"] = out["enstrophy_input"] / ll
    if strang_splitting is not None:
        out["enstrophy_dissipation"] = -2 * (strang_splitting.nu * ll + strang_splitting.alpha) * Z
        out["energy_dissipation"] = out["enstrophy_dissipation"] / ll
    if coeffs is not None:
        out["coefficients"] = {"omega": coeffs[0], "tendency": coeffs[1]}
        if has_forcing:
            out["coefficients"]["forcing"] = coeffs[2]
    return out


def _check_budget_mode(what):
    from . import integrators
    if not (integrators._SKEW_HERM_ and _laplacian._SKEW_HERM_):
        raise NotImplementedError("%s needs the skew-Hermitian mode (select_skewherm(True)): the advective tendency is "
                                  "formed as PW - (PW)^H" % what)


def _budget_call(ctx, W, nmax, has_forcing, strang_splitting, coefficients):
    """qf_spectral_budget on `ctx` (its transform mode set by the caller) for the host matrix W, or None: the resident state."""
    rows = np.zeros((3, nmax), dtype=np.float64)
    coeffs = np.zeros((3, nmax * nmax), dtype=np.float64) if coefficients else None
    _lib.check(ctx._lib.qf_spectral_budget(ctx.handle, None if W is None else ptr(W), nmax, ptr(rows),
                                           None if coeffs is None else ptr(coeffs)))
    return _budget_dict(rows, has_forcing, strang_splitting, coeffs)


def _spectrum_call(ctx, W, N):
    """Z_l, l = 0..N-1, of the host matrix W or (None) the resident state: qf_degree_spectrum."""
    Z = np.zeros(N, dtype=np.float64)
    _lib.check(ctx._lib.qf_degree_spectrum(ctx.handle, None if W is None else ptr(W), N, ptr(Z)))
    return Z


def spectral_budget(W, hamiltonian=None, forcing=None, strang_splitting=None, lmax=None, coefficients=False, streamed=None):
    """The per-degree budget of the state W on the device, from ONE sweep of the quantization basis (qf_spectral_budget).

    With P = hamiltonian(W) (the built-in solve_poisson, or a TridiagonalHamiltonian installed for the call), the
    advective tendency A = [P, W]/hbar and F = forcing(P, W) (an AffineForcing installed for the call), and omega, a, f =
    mat2shr of W, A, F band-limited to degrees el < lmax (default N), the result is a dict for el = 1..lmax-1:

        el                                       the degrees
        enstrophy, energy                        Z_l = sum_m omega_lm^2 and Z_l / (el (el+1))
        enstrophy_transfer, energy_transfer      T_l = 2 sum_m omega_lm a_lm and T_l / (el (el+1))
        enstrophy_flux, energy_flux              -cumsum of the transfers
        enstrophy_input, energy_input            I_l = 2 sum_m omega_lm f_lm and its energy form (with a forcing)
        enstrophy_dissipation, energy_dissipation  -2 (nu el (el+1) + alpha) Z_l and its energy form (with
                                                 strang_splitting=ViscDampStep(nu, alpha); host arithmetic)
        coefficients                             {"omega", "tendency", "forcing"} (coefficients=True): each equals
                                                 mat2shr of that matrix bit for bit

    sum(enstrophy)/2 is the enstrophy and sum(energy)/2 the Euler energy of W (el = 0 carries none for a traceless state);
    sum(enstrophy_transfer) vanishes to rounding for any Hamiltonian, sum(energy_transfer) for the built-in one.
    complex128 W in skew-Hermitian mode; `streamed` as in mat2shr."""
    from .context import as_c128
    from .quantization import _transform_context
    from .integrators import _is_native_hamiltonian, _hamiltonian_on, _forcing_on
    Wa = np.asarray(W)
    if Wa.dtype == np.complex64:
        raise NotImplementedError("spectral_budget of a complex64 W: the budget is double only; convert to complex128")
    Wc = as_c128(Wa, "W")
    N = Wc.shape[0]
    nmax = _band_limit(N, lmax)
    _check_budget_mode("spectral_budget")
    ham = None
    if isinstance(hamiltonian, _laplacian.TridiagonalHamiltonian) and _laplacian.installable(hamiltonian):
        hamiltonian.check_size(N)
        ham = hamiltonian
    elif not _is_native_hamiltonian(hamiltonian):
        raise TypeError("spectral_budget takes the built-in Hamiltonian or a TridiagonalHamiltonian")
    if forcing is not None:
        if not isinstance(forcing, _laplacian.AffineForcing):
            raise TypeError("spectral_budget takes an AffineForcing (a StochasticForcing's affine terms: on the "
                            "DeviceTrajectory that carries it)")
        forcing.check_size(N)
    if strang_splitting is not None and not isinstance(strang_splitting, _laplacian.ViscDampStep):
        raise TypeError("spectral_budget takes strang_splitting=ViscDampStep(nu, alpha) for the dissipation")
    ctx = _transform_context(N, None, streamed)
    with _hamiltonian_on(ctx, ham), _forcing_on(ctx, forcing):
        return _budget_call(ctx, Wc, nmax, forcing is not None, strang_splitting, coefficients)


MHD_COEFFICIENTS = ("omega", "theta", "advection", "lorentz", "induction")


def _mhd_budget_dict(rows, coeffs=None):
    """The MHD budget's dictionary from the device's rows (9, Nmax) of qf_mhd_spectral_budget, l = 0..Nmax-1: host arithmetic
    only, in the style of `_budget_dict`.  Everything is reported for el = 1..Nmax-1; with ll = el (el + 1) the kinetic
    forms divide by ll, the magnetic ones multiply by it, and a flux is minus the running sum of its transfer."""
    rows = np.asarray(rows, dtype=np.float64)
    nmax = rows.shape[1]
    el = np.arange(1, nmax)
    ll = (el * (el + 1)).astype(np.float64)
    r = [rows[i, 1:].copy() for i in range(9)]
    out = {"el": el,
           "enstrophy": r[0], "kinetic_energy": r[0] / ll,
           "magnetic_potential": r[1], "magnetic_energy": ll * r[1],
           "cross_helicity": r[2],
           "kinetic_transfer_advection": r[3] / ll, "kinetic_transfer_lorentz": r[4] / ll,
           "magnetic_transfer": ll * r[5],
           "enstrophy_transfer_advection": r[3], "enstrophy_source_lorentz": r[4],
           "potential_transfer": r[5],
           "cross_helicity_transfer": r[6] + r[7] + r[8]}
    out["energy"] = out["kinetic_energy"] + out["magnetic_energy"]
    out["energy_transfer"] = out["kinetic_transfer_advection"] + out["kinetic_transfer_lorentz"] + out["magnetic_transfer"]
    for flux, transfer in (("kinetic_flux_advection", "kinetic_transfer_advection"), ("energy_flux", "energy_transfer"),
                           ("potential_flux", "potential_transfer"), ("cross_helicity_flux", "cross_helicity_transfer"),
                           ("enstrophy_flux_advection", "enstrophy_transfer_advection")):
        out[flux] = -np.cumsum(out[transfer])
    if coeffs is not None:
        out["coefficients"] = dict(zip(MHD_COEFFICIENTS, coeffs))
    return out


def _mhd_budget_call(ctx, nmax, coefficients):
    """qf_mhd_spectral_budget on `ctx` (its transform mode set by the caller) for the resident pair."""
    rows = np.zeros((9, nmax), dtype=np.float64)
    coeffs = np.zeros((5, nmax * nmax), dtype=np.float64) if coefficients else None
    _lib.check(ctx._lib.qf_mhd_spectral_budget(ctx.handle, nmax, ptr(rows), None if coeffs is None else ptr(coeffs)))
    return _mhd_budget_dict(rows, coeffs)


def mhd_spectral_budget(state, lmax=None, coefficients=False, streamed=None):
    """The per-degree budget of the MHD pair state = (W, Theta), a (2,N,N) complex128 array, on the device, from ONE sweep of
    the quantization basis (qf_mhd_spectral_budget).  The system is quflow/integrators/mhd.py's with hamiltonian = solve_mhd:

        P = Delta^-1 W,  B = Delta Theta,   W' = ([P, W] + [B, Theta]) / hbar,   Theta' = [P, Theta] / hbar.

    With omega, theta, a, b, c = mat2shr of W, Theta, [P,W]/hbar (advection), [B,Theta]/hbar (the Lorentz term),
    [P,Theta]/hbar (induction), band-limited to degrees el < lmax (default N), and ll = el (el + 1), the result is a dict
    for el = 1..lmax-1 (sums over m):

        el                              the degrees
        enstrophy, kinetic_energy       sum omega^2 and the same / ll
        magnetic_potential, magnetic_energy   sum theta^2 (the mean-square potential) and ll times it
        energy                          kinetic_energy + magnetic_energy
        cross_helicity                  sum omega theta
        kinetic_transfer_advection, kinetic_transfer_lorentz   2 sum omega a / ll and 2 sum omega b / ll
        magnetic_transfer               ll 2 sum theta c
        energy_transfer                 the sum of those three
        enstrophy_transfer_advection    2 sum omega a
        enstrophy_source_lorentz        2 sum omega b: the Lorentz term does not conserve enstrophy -- a source, no flux
        potential_transfer              2 sum theta c
        cross_helicity_transfer         sum theta a + sum theta b + sum omega c
        kinetic_flux_advection, energy_flux, potential_flux, cross_helicity_flux, enstrophy_flux_advection
                                        -cumsum of the matching transfer
        coefficients                    {"omega", "theta", "advection", "lorentz", "induction"} (coefficients=True): each
                                        equals mat2shr of that matrix bit for bit

    sum(kinetic_energy)/2, sum(magnetic_energy)/2, sum(magnetic_potential)/2, sum(cross_helicity) and sum(enstrophy)/2 are
    energy_kinetic, energy_magnetic, magnetic_casimir, cross_helicity and enstrophy of `physics.mhd_diagnostics`.  These
    vanish to rounding: sum(kinetic_transfer_advection), sum(kinetic_transfer_lorentz + magnetic_transfer),
    sum(potential_transfer), sum(cross_helicity_transfer), sum(enstrophy_transfer_advection).
    Skew-Hermitian mode; `streamed` as in mat2shr."""
    from .quantization import _transform_context
    state = np.asarray(state)
    if state.dtype == np.complex64:
        raise NotImplementedError("mhd_spectral_budget of a complex64 state: the budget is double only; convert to "
                                  "complex128")
    if state.ndim != 3 or state.shape[0] != 2 or state.shape[1] != state.shape[2]:
        raise ValueError("the MHD state must be a (2,N,N) array (W, Theta), got shape %s" % (state.shape,))
    N = state.shape[-1]
    nmax = _band_limit(N, lmax)
    _check_budget_mode("mhd_spectral_budget")
    sc = np.ascontiguousarray(state, dtype=np.complex128)
    ctx = _transform_context(N, None, streamed)
    _lib.check(ctx._lib.qf_states_upload(ctx.handle, ptr(sc), 2))
    return _mhd_budget_call(ctx, nmax, coefficients)


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
