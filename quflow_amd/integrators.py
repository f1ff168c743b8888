"""Isospectral midpoint stepper of quflow on the MI355X.

`isomp` keeps the stepper signature of quflow.integrators.isomp
(= isomp_fixedpoint, quflow/integrators/isospectral.py:338-353,617) so that
`quflow.simulation.solve(..., integrator=quflow_amd.isomp)` (simulation.py:788) and
the reference's notebooks drive it unchanged.  `IsompHIP(N, dtype)` has the
constructor/call shape of the reference's device precedent `IsompCUDA`
(quflow/experimental/isospectral_cuda.py:52-80,120-137) for the runfile selection of
quflow/simulation.py:554-562.

The whole call -- Poisson solves, both complex GEMMs, the fused commutator epilogue,
residual norms and the W update -- runs in hand-written HIP kernels behind one C-ABI
call (qf_isomp).  There is no CPU path: without the library or a GPU this raises.
"""
import contextlib
import ctypes
import operator

import numpy as np

from . import _lib
from . import laplacian as _laplacian
from .context import Context, default_device, get_context, get_stepper_context, ptr, stepper_context
from .geometry import hbar


_SKEW_HERM_ = True


def _device_matmul(A, B):
    from .geometry import _device_matmul as mm
    return mm(A, B)


def _device_commutator(W, P, skewherm):
    """qf_commutator: product(s) and the elementwise subtraction on the device, one PCIe round trip."""
    from . import _lib
    from .context import as_c128, get_context, ptr, result_array
    Wc = as_c128(W, "W")
    Pc = as_c128(P, "P")
    if Wc.shape != Pc.shape:
        raise ValueError("operands could not be broadcast together with shapes %s %s" % (Wc.shape, Pc.shape))
    C = result_array(Wc.shape, Wc.dtype, "commutator")
    ctx = get_context(Wc.shape[-1])
    _lib.check(ctx._lib.qf_commutator(ctx.handle, ptr(Wc), ptr(Pc), ptr(C), int(bool(skewherm))))
    return C


def commutator_generic(W, P):
    """W@P - P@W for arbitrary matrices (quflow/integrators/isospectral.py:22-36): both products and the subtraction
    on the device (the bits of the two products followed by numpy's `VF -= ...`)."""
    return _device_commutator(W, P, False)


def commutator_skewherm(W, P):
    """W@P - (W@P)^H: the commutator of skew-Hermitian matrices from ONE product
    (quflow/integrators/isospectral.py:39-54) -- the product and the conjugate subtraction the reference does on the host
    (`VF -= VF.conj().T`) both on the device: x - conj(y) is one exact negation and one rounding either way."""
    return _device_commutator(W, P, True)


# the default commutator (isospectral.py:57); select_skewherm switches it (:109-116)
commutator = commutator_skewherm


def project_skewherm(W):
    """In-place projection onto the skew-Hermitian matrices (isospectral.py:60-63)."""
    W /= 2.0
    W -= W.conj().T


def select_skewherm(flag):
    """quflow/integrators/isospectral.py:96-118: whether the integrators may assume skew-Hermitian
    matrices (commutator as PW - PW^H instead of PW - W@P); also switches the default `commutator`
    and the Laplacian backend."""
    global _SKEW_HERM_, commutator
    _SKEW_HERM_ = bool(flag)
    commutator = commutator_skewherm if flag else commutator_generic
    _laplacian.select_skewherm(flag)


def estimate_stepsize(W, P=None, safety_factor=0.1):
    """safety_factor * pi / lambda_max(P) with P = solve_poisson(W) (the device solve) unless given, and
    lambda_max the spectral norm (quflow/integrators/isospectral.py:121-148, geometry.norm_Linf).  The
    stepsize is dimension-free: delta_time = stepsize * hbar(N)."""
    from .geometry import norm_Linf
    if P is None:
        P = _laplacian.solve_poisson(W)
    lambda_max = norm_Linf(P)
    return safety_factor * np.pi / lambda_max


def _is_native_hamiltonian(h):
    """The built-in Hamiltonian P = Delta^-1 W: ours, a PoissonHIP, or the reference's own
    default `quflow.laplacian.cpu.solve_poisson`, which simulation.solve injects when the
    user gives none (quflow/simulation.py:728-729)."""
    if h is None or h is _laplacian.solve_poisson or isinstance(h, _laplacian.PoissonHIP):
        return True
    mod = getattr(h, "__module__", "") or ""
    return getattr(h, "__name__", "") == "solve_poisson" and (
        mod.startswith("quflow.laplacian") or mod.startswith("quflow_amd.laplacian"))


def _installable(h, W):
    """`h` if it is a TridiagonalHamiltonian that this call installs on its device context -- skew-Hermitian mode,
    complex128 data -- else None (the instance is then the foreign callable it also is)."""
    if (_laplacian.installable(h) and _SKEW_HERM_ and isinstance(W, np.ndarray) and W.dtype == np.complex128):
        h.check_size(W.shape[-1])
        return h
    return None


def _stepper_context(N, device):
    """The stepper context of one hooked call, held for the call (context.stepper_context): a hooked stepper called from
    inside one of this call's hooks gets a further context and leaves this call's trajectory alone."""
    return stepper_context(N, device, get_stepper_context)


@contextlib.contextmanager
def _hamiltonian_on(ctx, ham):
    """The call's Hamiltonian installed on its context for the call alone: the cached per-N contexts are shared, and a
    later default call must find the built-in Hamiltonian again -- also after an error."""
    if ham is None:
        yield
        return
    ham.install(ctx)
    try:
        yield
    finally:
        ham.uninstall(ctx)


def _refuse_stochastic(forcing, who):
    """A StochasticForcing is never dropped or run as something else: the routes that do not follow it say so."""
    if isinstance(forcing, _laplacian.StochasticForcing):
        raise NotImplementedError("%s: %s" % (who, _laplacian._STOCHASTIC_ROUTES))


def _installable_forcing(f, W):
    """`f` if it is an AffineForcing or a StochasticForcing that this call installs on its device context -- skew-Hermitian mode, one (N,N)
    complex128 state -- else None (the instance is then the host callable `forcing(P, W)` it also is)."""
    if (_laplacian.forcing_installable(f) and _SKEW_HERM_ and isinstance(W, np.ndarray) and W.ndim == 2
            and W.shape[0] == W.shape[1] and W.dtype == np.complex128):
        f.check_size(W.shape[-1])
        return f
    return None


@contextlib.contextmanager
def _forcing_on(ctx, aff):
    """The call's AffineForcing / StochasticForcing installed on its context for the call alone (the twin of
    _hamiltonian_on): a later call on the cached context must find no forcing again -- also after an error.  A
    StochasticForcing takes its counter back from the context before it leaves (the steps the call ran)."""
    if aff is None:
        yield
        return
    aff.install(ctx)
    try:
        yield
    finally:
        try:
            if isinstance(aff, _laplacian.StochasticForcing):
                aff.sync(ctx)
        finally:
            aff.uninstall(ctx)


def _check_iterations(minit, maxit):
    """AssertionError like isospectral.py:400-401 (and mhd.py), for every fixed-point stepper and resident `advance`."""
    assert minit >= 1, "minit must be at least 1."
    assert maxit >= minit, "maxit must be at minit."


def _tol_arg(tol):
    """The `tol` argument as the float of the C entries: 'auto' and negative values mean the automatic tolerance (a negative
    float goes through as it is, isospectral.py:440); any other string is the reference's TypeError."""
    if isinstance(tol, str):
        if tol != 'auto':
            raise TypeError("tol must be a float or 'auto' (the reference compares it with a number: '<' not supported between instances of 'str' and 'int')")
        return -1.0
    return float(tol)


def _report_iterations(stats, verbatim, st, steps, maxit_key='number_of_maxit'):
    """The per-step averages of a call (isospectral.py:609-611, mhd.py:451-453): printed with `verbatim`, written into `stats`
    unless it is None; nothing for an empty call."""
    if steps <= 0:
        return
    if verbatim:
        print("Average number of iterations per step: {:.2f}".format(st.total_iterations / steps))
    if stats is not None:
        stats["iterations"] = st.total_iterations / steps
        stats[maxit_key] = st.number_of_maxit / steps


def _report(stats, verbatim, st, steps, auto, tol_report, tol_key='tol_auto', maxit_key='number_of_maxit'):
    """What a fixed-point stepper says after its C call: with an automatic tolerance "Tolerance set to" and stats[tol_key]
    (isospectral.py:451-452; `tol_report` where the host computed it, else what the device used), then the averages.  `stats`
    is written only if truthy, as the reference tests it.  The differences between the steppers are kept as they were:
      * _isomp_stepwise_on reports the tolerance before its loop, from the host formula (_report_tolerance), and the averages
        of its own sums after it;
      * magmp's keys are 'tol' and 'maxit' (mhd.py:341,452-454);
      * isomp_quasinewton writes stats['tol'] always and tests `stats is not None`: it uses _report_iterations alone."""
    if auto:
        _report_tolerance(stats, verbatim, st.tol_used if tol_report is None else tol_report, tol_key)
    _report_iterations(stats if stats else None, verbatim, st, steps, maxit_key)


def _report_tolerance(stats, verbatim, tol_used, tol_key='tol_auto'):
    """The automatic tolerance of a call (isospectral.py:451-452): printed with `verbatim`, written into a truthy `stats`."""
    if verbatim:
        print("Tolerance set to {}.".format(tol_used))
    if stats:
        stats[tol_key] = tol_used


def _stats_dict(st, steps):
    """The statistics a resident `advance` returns (bench.py and the tools read these keys)."""
    return {"iterations": st.total_iterations / max(steps, 1), "number_of_maxit": st.number_of_maxit / max(steps, 1),
            "total_iterations": st.total_iterations, "tol": st.tol_used, "last_resnorm": st.last_resnorm}


def isomp_fixedpoint(W,
                     dt,
                     steps=100,
                     hamiltonian=_laplacian.solve_poisson,
                     time=None,
                     forcing=None,
                     strang_splitting=None,
                     stats=None,
                     callback=None,
                     tol='auto',
                     maxit=10,
                     minit=1,
                     verbatim=False,
                     compsum=False,
                     reinitialize=False,
                     device=None):
    """Isospectral midpoint method with fixed-point iterations for skew-Hermitian W
    (quflow/integrators/isospectral.py:338-613).  `W` (host ndarray, complex128 (N,N)) is
    overwritten and returned, like the reference (isospectral.py:361-362,592,613).

    Everything stays on the device for hamiltonian = solve_poisson (the default) with tol, maxit,
    minit, compsum, reinitialize, stats, verbatim, time (autonomous: ignored, as the reference
    does for a Hamiltonian without a `time` argument, isospectral.py:416-423).

    The host hooks of the reference run as host hooks here too, around a trajectory that stays on the
    device (a context of its own: a hook may call solve_poisson, energy_euler, ... freely):
      * `strang_splitting(dt/2, W)` (isospectral.py:466-467, 598-599) and `callback(W, dW)`
        (:549-550) with the built-in Hamiltonian: the fused device stepper one step at a time (qf_isomp,
        then qf_isomp_continue: the iteration vector carries over as inside one reference call), the
        state crosses PCIe around each hook.  The callback gets host copies.
      * `forcing(P, W[, time])` (:512-520, 591-595), a foreign `hamiltonian(W[, time])` (:488-492), the
        general commutator of select_skewherm(False) (:504-505), and hooks / compsum on (k,N,N) stacks:
        qf_isomp_hooked -- W, dW, Whalf, the products and the Kahan term never leave the device; per
        iteration only what the hook reads goes down and what it returns comes up.
      * `forcing=AffineForcing(...)` on an (N,N) complex128 state in skew-Hermitian mode is no host hook: it is installed
        on the device context for the call and one kernel forms the force term inside that loop (nothing crosses PCIe
        for it); a TridiagonalHamiltonian and a ViscDampStep are followed on the device next to it.
    """
    _check_iterations(minit, maxit)

    # a TridiagonalHamiltonian is followed on the device (installed for this call): native in every route below
    ham = _installable(hamiltonian, W)
    native = ham is not None or _is_native_hamiltonian(hamiltonian)
    # `for k in range(steps)` and the in-place complex updates (isospectral.py:463, 481-482, 592): a float step count and a real
    # or integer W are TypeErrors, a negative count an empty loop -- a real W is not silently advanced and truncated here either
    steps = _reference_args(W, steps)
    if steps == 0 and not np.issubdtype(W.dtype, np.complexfloating):
        return W                 # the reference's empty loop never touches a real / integer W
    stacked = W.ndim == 3
    hooks = strang_splitting is not None or callback is not None
    if (forcing is not None or not native or not _SKEW_HERM_ or not _laplacian._SKEW_HERM_
            or (stacked and (hooks or compsum))):
        # hooks that act inside an iteration, the general (not skew-Hermitian) commutator, and hooks /
        # compsum on stacks: device-resident state with host hooks (qf_isomp_hooked)
        return _isomp_hooked(W, dt, steps, hamiltonian, native, time, forcing, strang_splitting, stats, callback,
                             tol, maxit, minit, verbatim, compsum, reinitialize, device, ham=ham)
    if hooks:
        return _isomp_stepwise(W, dt, steps, strang_splitting, stats, callback, tol, maxit, minit, verbatim,
                               compsum, reinitialize, device, ham=ham)

    if not isinstance(W, np.ndarray):
        raise TypeError("W must be a numpy ndarray")
    if W.ndim == 3 and W.shape[-1] == W.shape[-2]:
        # a stack of states: P from state 0, the exit test on state 0 (isospectral.py:527-532)
        return _isomp_states(W, dt, steps, tol, minit, maxit, reinitialize, False, stats, verbatim, device,
                             tol_key='tol_auto', maxit_key='number_of_maxit', ham=ham)
    if W.ndim != 2 or W.shape[0] != W.shape[1]:
        raise ValueError("W must be a square matrix or a (k,N,N) stack")
    N = W.shape[-1]
    ctx = get_context(N, device)

    auto = isinstance(tol, str) or tol < 0      # negative => auto (isospectral.py:440)
    tol_c, tol_report = _device_tol(W, dt, tol, compsum)

    st = _lib.IsompStats()
    if W.dtype == np.complex64 and _laplacian.single_precision_on_device():
        # complex64 data is advanced in single precision, as the reference does it: float32 Poisson solve,
        # complex64 products, float32 Kahan term; the tolerance above is the reference's float32 rule
        Wc = np.ascontiguousarray(W)
        _lib.check(ctx._lib.qf_c64_upload_W(ctx.handle, ptr(Wc)))
        _lib.check(ctx._lib.qf_c64_isomp(ctx.handle, float(dt), int(steps), tol_c, int(minit), int(maxit),
                                         int(bool(compsum)), int(bool(reinitialize)), ctypes.byref(st)))
        _lib.check(ctx._lib.qf_c64_download_W(ctx.handle, ptr(Wc)))
    else:
        Wc = np.ascontiguousarray(W, dtype=np.complex128)
        with _hamiltonian_on(ctx, ham):
            _lib.check(ctx._lib.qf_upload_W(ctx.handle, ptr(Wc)))
            _lib.check(ctx._lib.qf_isomp(ctx.handle, float(dt), int(steps), tol_c, int(minit), int(maxit),
                                         int(bool(compsum)), int(bool(reinitialize)), ctypes.byref(st)))
            _lib.check(ctx._lib.qf_download_W(ctx.handle, ptr(Wc)))
    if Wc is not W:
        W[...] = Wc                  # in-place contract

    _report(stats, verbatim, st, steps, auto, tol_report)
    return W


def _auto_tol(W, dt, compsum):
    """isospectral.py:440-452: the machine epsilon is that of W.dtype (complex64 input: float32)."""
    W0 = W[(0,) * (W.ndim - 2) + (Ellipsis,)] if W.ndim > 2 else W
    dtype = W.dtype if W.dtype == np.complex64 else np.float64
    mach_eps = np.finfo(dtype).eps
    if not compsum:
        mach_eps = np.sqrt(mach_eps)
    return (mach_eps * dt / hbar(W.shape[-1])) * np.linalg.norm(W0, np.inf)


def _device_tol(W, dt, tol, compsum):
    """(tol for the C entry, tolerance to report or None).  A negative tol asks the device for the
    automatic double-precision tolerance (read back as stats.tol_used); complex64 input gets the
    reference's single-precision tolerance, evaluated here from the input, so that a complex64 run stops
    where the reference's does although the arithmetic on the device is double precision."""
    tol = _tol_arg(tol)
    if tol < 0 and W.dtype == np.complex64:
        t = float(_auto_tol(W, dt, compsum))
        return t, t
    return tol, None


def _isomp_stepwise(W, dt, steps, strang_splitting, stats, callback, tol, maxit, minit, verbatim, compsum,
                    reinitialize, device, ham=None):
    if not isinstance(W, np.ndarray) or W.ndim != 2 or W.shape[0] != W.shape[1]:
        raise ValueError("W must be a square matrix")
    _tol_arg(tol)
    # (an installed TridiagonalHamiltonian: the same loop, on the same stepper context, with it in force)
    with _stepper_context(W.shape[-1], device) as ctx, _hamiltonian_on(ctx, ham):
        return _isomp_stepwise_on(W, dt, steps, strang_splitting, stats, callback, tol, maxit, minit, verbatim, compsum,
                                  reinitialize, ctx)


def _isomp_stepwise_on(W, dt, steps, strang_splitting, stats, callback, tol, maxit, minit, verbatim, compsum,
                       reinitialize, ctx):
    """strang_splitting / callback around device steps (built-in Hamiltonian): one step per
    qf_isomp / qf_isomp_continue call, the tolerance fixed once from the initial state as in the
    reference (isospectral.py:440-452)."""
    N = W.shape[-1]
    tol_c = _tol_arg(tol)
    # (`ctx`: the call's stepper context -- the hooks may use the shared context (solve_viscdamp, energy_euler, ...) and
    # call hooked steppers of their own)
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    if tol_c < 0:
        tol_c = float(_auto_tol(W, dt, compsum))
        _report_tolerance(stats, verbatim, tol_c)         # (known before the loop)
    st, total = _lib.IsompStats(), _lib.IsompStats()      # (one step's record; the call's sums, for the report)
    PW = np.zeros((N, N), dtype=np.complex128) if callback is not None else None
    on_device = False
    resident_strang = isinstance(strang_splitting, _laplacian.ViscDampStep)
    for k in range(steps):
        if resident_strang:                       # the half step on the resident state
            if not on_device:
                _lib.check(ctx._lib.qf_upload_W(ctx.handle, ptr(Wc)))
                on_device = True
            strang_splitting.apply_resident(ctx, dt / 2)
            if callback is not None:
                _lib.check(ctx._lib.qf_download_W(ctx.handle, ptr(Wc)))
        elif strang_splitting:
            if on_device:
                _lib.check(ctx._lib.qf_download_W(ctx.handle, ptr(Wc)))
            Wc = np.ascontiguousarray(strang_splitting(dt / 2, Wc), dtype=np.complex128)
            on_device = False
        elif callback is not None and on_device:
            _lib.check(ctx._lib.qf_download_W(ctx.handle, ptr(Wc)))      # the callback's W: before the update
        if not on_device:
            _lib.check(ctx._lib.qf_upload_W(ctx.handle, ptr(Wc)))
            on_device = True
        step = ctx._lib.qf_isomp if k == 0 else ctx._lib.qf_isomp_continue
        _lib.check(step(ctx.handle, float(dt), 1, float(tol_c), int(minit), int(maxit), int(bool(compsum)),
                        int(bool(reinitialize)), ctypes.byref(st)))
        total.total_iterations += st.total_iterations
        total.number_of_maxit += st.number_of_maxit
        if callback is not None:
            # PWcomm of the last iteration, doubled (isospectral.py:547-550), from the device's PW
            _lib.check(ctx._lib.qf_download_buffer(ctx.handle, _lib.BUFFER_IDS["PW"], ptr(PW)))
            callback(Wc.copy(), 2.0 * (PW - PW.conj().T))
        if resident_strang:
            strang_splitting.apply_resident(ctx, dt / 2)
        elif strang_splitting:
            _lib.check(ctx._lib.qf_download_W(ctx.handle, ptr(Wc)))
            Wc = np.ascontiguousarray(strang_splitting(dt / 2, Wc), dtype=np.complex128)
            on_device = False
    if on_device:
        _lib.check(ctx._lib.qf_download_W(ctx.handle, ptr(Wc)))
    W[...] = Wc
    _report(stats, verbatim, total, steps, False, None)
    return W


def _probe_time(fn, args, time):
    """The reference finds out whether a hook is time dependent by calling it once with `time=`
    (isospectral.py:403-423): a TypeError means autonomous.  Returns (takes_time, what that call returned or None)."""
    if time is None:
        return False, None
    try:
        out = fn(*args, time=time)
    except TypeError:
        return False, None
    return True, out


def _takes_time(fn, args, time):
    return _probe_time(fn, args, time)[0]


class _HookTable:
    """qf_isomp_hooks for a set of Python hooks: C callbacks over numpy views of the library's pinned
    staging matrices.  An exception raised by a hook is kept and re-raised once the C call has returned."""

    def __init__(self, N, k, squeeze):
        self.N, self.k, self.squeeze = N, k, squeeze
        self.error = None
        self.c = _lib.IsompHooks()
        self.c.skewh = int(bool(_SKEW_HERM_))
        self.c.solve_skewh = int(bool(_laplacian._SKEW_HERM_))
        self._keep = []

    def _view(self, p, k):
        buf = (ctypes.c_double * (2 * k * self.N * self.N)).from_address(p)
        a = np.frombuffer(buf, dtype=np.complex128).reshape(k, self.N, self.N)
        return a[0] if self.squeeze else a

    def _guard(self, body):
        def run(*args):
            try:
                body(*args)
                return 0
            except BaseException as exc:      # noqa: BLE001 -- carried across the C frame
                self.error = exc
                return 1
        return run

    def set_hamiltonian(self, fn, takes_time, per_state=False):
        """`per_state`: False = one (N,N) stream matrix for all states; True = one per state, a (k,N,N) array
        (np.matmul batches the products); None = a stack whose Hamiltonian has not said yet: qf_isomp_hooks::states_p
        goes out as -1 and the FIRST evaluation the stepper itself asks for settles it (the library reads the field
        back after that call) -- no entry probe, so the user's function is called exactly as often as the reference
        calls it, whatever runs before the first evaluation (Strang half step, a carried increment)."""
        state = {"per_state": per_state}
        def body(user, pW, pP, t):
            W = self._view(pW, self.k)
            P = np.asarray(fn(W, time=t) if takes_time else fn(W))
            if state["per_state"] is None:
                if P.shape not in ((self.N, self.N), (1, self.N, self.N), (self.k, self.N, self.N)):
                    raise ValueError("the Hamiltonian returned a %s array for a (%d,%d,%d) stack: neither one (N,N) stream matrix "
                                     "for all states nor one per state" % (P.shape, self.k, self.N, self.N))
                state["per_state"] = (P.shape == (self.k, self.N, self.N) and self.k > 1)
                self.c.states_p = int(state["per_state"])
            if P.shape == (1, self.N, self.N) and not state["per_state"]:
                P = P.reshape(self.N, self.N)       # (numpy broadcasts a (1,N,N) stream matrix over the stack)
            if state["per_state"]:
                if P.shape != (self.k, self.N, self.N):
                    raise ValueError("the Hamiltonian returned a %s array after a (%d,%d,%d) one" % (P.shape, self.k, self.N, self.N))
                np.frombuffer((ctypes.c_double * (2 * self.k * self.N * self.N)).from_address(pP),
                              dtype=np.complex128).reshape(self.k, self.N, self.N)[...] = P
                return
            if P.shape != (self.N, self.N):
                # (numpy raises ValueError where the reference multiplies or stores it: isospectral.py:496-509)
                raise ValueError("the Hamiltonian returned a %s array for (%d,%d) states: operands could not be broadcast "
                                 "together" % (P.shape, self.N, self.N))
            self._view(pP, 1).reshape(self.N, self.N)[...] = P
        self.c.states_p = -1 if per_state is None else int(bool(per_state))
        cb = _lib.HAMILTONIAN_CB(self._guard(body))
        self._keep.append(cb)
        self.c.hamiltonian = cb
        self.c.hamiltonian_takes_time = int(takes_time)

    def set_hamiltonian_pair(self, fn, takes_time):
        """magmp: `hamiltonian(state[, time])` returns the pair (P, B) (mhd.py:10-18, 371-374)."""
        def body(user, pW, pPB, t):
            state = self._view(pW, 2)
            P, B = fn(state, time=t) if takes_time else fn(state)
            out = self._view(pPB, 2)
            out[0][...] = P
            out[1][...] = B
        cb = _lib.HAMILTONIAN_CB(self._guard(body))
        self._keep.append(cb)
        self.c.hamiltonian = cb
        self.c.hamiltonian_takes_time = int(takes_time)

    def set_forcing(self, fn, takes_time):
        def body(user, pP, pW, pF, t):
            if self.c.states_p:       # the Hamiltonian returns one stream matrix per state: forcing sees them all
                P = np.frombuffer((ctypes.c_double * (2 * self.k * self.N * self.N)).from_address(pP),
                                  dtype=np.complex128).reshape(self.k, self.N, self.N)
            else:
                P = self._view(pP, 1).reshape(self.N, self.N)
            W = self._view(pW, self.k)
            F = fn(P, W, time=t) if takes_time else fn(P, W)
            self._view(pF, self.k)[...] = F
        cb = _lib.FORCING_CB(self._guard(body))
        self._keep.append(cb)
        self.c.forcing = cb
        self.c.forcing_takes_time = int(takes_time)

    def set_strang(self, fn):
        def body(user, h, pW):
            W = self._view(pW, self.k)
            W[...] = fn(h, W)
        cb = _lib.STRANG_CB(self._guard(body))
        self._keep.append(cb)
        self.c.strang = cb

    def set_strang_table(self, table, key):
        table = np.ascontiguousarray(table, dtype=np.float64)
        self._keep.append(table)
        self.c.strang_table = table.ctypes.data
        self.c.strang_key = key

    def set_callback(self, fn):
        def body(user, pW, pD):
            fn(self._view(pW, self.k), self._view(pD, self.k))
        cb = _lib.CALLBACK_CB(self._guard(body))
        self._keep.append(cb)
        self.c.callback = cb

    def check(self, rc):
        if self.error is not None:
            err, self.error = self.error, None
            raise err
        if rc == 6:          # QF_ERR_UNSUPPORTED: what the reference raises NotImplementedError for
            raise NotImplementedError(_lib.load().qf_last_error().decode("utf-8", "replace"))
        _lib.check(rc)


def _isomp_hooked(W, dt, steps, hamiltonian, native, time, forcing, strang_splitting, stats, callback, tol,
                  maxit, minit, verbatim, compsum, reinitialize, device, ham=None):
    """isomp_fixedpoint with hooks inside the iteration (forcing, foreign Hamiltonian), the general
    commutator, or hooks / compsum on a stack of states: qf_isomp_hooked keeps the trajectory on the
    device and calls back for what only Python can compute."""
    if W.ndim not in (2, 3) or W.shape[-1] != W.shape[-2]:
        raise ValueError("W must be a square matrix or a (k,N,N) stack")
    _tol_arg(tol)
    N = W.shape[-1]
    squeeze = W.ndim == 2
    k = 1 if squeeze else W.shape[0]
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    table = _HookTable(N, k, squeeze)
    aff = _installable_forcing(forcing, W)        # installed on the device for this call: no forcing hook
    if aff is None:
        _refuse_stochastic(forcing, "isomp on a stack, on complex64 data or with select_skewherm(False)")
    if forcing is not None and aff is None:
        table.set_forcing(forcing, _takes_time(forcing, (Wc, Wc), time))
    if not native:
        # one stream matrix for all states or one per state?  Not asked here: the stepper's first evaluation tells
        # (set_hamiltonian, per_state=None), so the user's function is called as often as the reference calls it --
        # the autonomy probe with `time=` included (isospectral.py:416-423), with or without Strang splitting
        table.set_hamiltonian(hamiltonian, _takes_time(hamiltonian, (Wc,), time), per_state=(False if squeeze or k == 1 else None))
    if isinstance(strang_splitting, _laplacian.ViscDampStep):
        tab, key = strang_splitting.table_and_key(N, dt / 2)
        table.set_strang_table(tab, key)
    elif strang_splitting is not None:
        table.set_strang(strang_splitting)
    if callback is not None:
        table.set_callback(callback)
    tol_c, tol_report = _device_tol(W, dt, tol, compsum)
    return _hooked_call(table, W, Wc, k, dt, steps, time, tol, tol_c, tol_report, minit, maxit, compsum, reinitialize, stats,
                        verbatim, device, 'tol_auto', 'number_of_maxit', ham=ham, aff=aff)


def _hooked_call(table, W, Wc, k, dt, steps, time, tol, tol_c, tol_report, minit, maxit, compsum, reinitialize, stats, verbatim,
                 device, tol_key, maxit_key, ham=None, aff=None):
    """What _isomp_hooked and _magmp_hooked share once their table is set up: the table's time fields, the stepper context,
    qf_isomp_hooked with the call's Hamiltonian / forcing installed, the hooks' exception or the library's error, the copy
    back into the caller's array and the report."""
    table.c.has_time = int(time is not None)
    table.c.time = float(time) if time is not None else 0.0
    auto = isinstance(tol, str) or tol < 0
    st = _lib.IsompStats()
    # (`native`: the device's own solve, of what is installed)
    with _stepper_context(W.shape[-1], device) as ctx, _hamiltonian_on(ctx, ham), _forcing_on(ctx, aff):
        rc = ctx._lib.qf_isomp_hooked(ctx.handle, ptr(Wc), k, float(dt), int(steps), tol_c, int(minit),
                                      int(maxit), int(bool(compsum)), int(bool(reinitialize)), ctypes.byref(table.c),
                                      ctypes.byref(st))
    table.check(rc)
    if Wc is not W:
        W[...] = Wc
    _report(stats, verbatim, st, steps, auto, tol_report, tol_key, maxit_key)
    return W


def _magmp_hooked(W, dt, steps, hamiltonian, native_mhd, time, forcing, stats, callback, tol, maxit, minit, verbatim,
                  reinitialize, device):
    """magmp_fixedpoint with host hooks (quflow/integrators/mhd.py:235-456): qf_isomp_hooked in its magnetic mode --
    the (2,N,N) state, dW, the products and the magnetic terms stay on the device; a foreign Hamiltonian returns the
    pair (P, B), `forcing(P, state)` a (2,N,N) force, `callback(state, 2 PWcomm)` host copies."""
    tol_c = _tol_arg(tol)
    if not (_SKEW_HERM_ and _laplacian._SKEW_HERM_):
        raise NotImplementedError("magmp on the HIP path is for skew-Hermitian matrices (select_skewherm(True)).")
    N = W.shape[-1]
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    table = _HookTable(N, 2, False)
    table.c.magnetic = 1
    if forcing is not None:
        table.set_forcing(forcing, _takes_time(forcing, (Wc, Wc), time))
    if not native_mhd:
        table.set_hamiltonian_pair(hamiltonian, _takes_time(hamiltonian, (Wc,), time))
    if callback is not None:
        table.set_callback(callback)
    # (the device's tolerance whatever the dtype; the keys of mhd.py:344-345, 451-453)
    return _hooked_call(table, W, Wc, 2, dt, steps, time, tol, -1.0 if tol_c < 0 else tol_c, None, minit, maxit, False,
                        reinitialize, stats, verbatim, device, 'tol', 'maxit')


def _isomp_states(W, dt, steps, tol, minit, maxit, reinitialize, magnetic, stats, verbatim, device,
                  tol_key, maxit_key, ham=None):
    """(k,N,N) isomp / magmp through qf_isomp_states; W overwritten and returned."""
    auto = isinstance(tol, str) or tol < 0
    tol_c, tol_report = _device_tol(W, dt, tol, False)
    k, N = W.shape[0], W.shape[-1]
    ctx = get_context(N, device)
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    st = _lib.IsompStats()
    with _hamiltonian_on(ctx, ham):
        _lib.check(ctx._lib.qf_isomp_states(ctx.handle, ptr(Wc), int(k), float(dt), int(steps), tol_c, int(minit),
                                            int(maxit), int(bool(reinitialize)), int(bool(magnetic)), ctypes.byref(st)))
    if Wc is not W:
        W[...] = Wc
    _report(stats, verbatim, st, steps, auto, tol_report, tol_key, maxit_key)
    return W


# Default isospectral method (isospectral.py:617)
isomp = isomp_fixedpoint


# -------------------------------------------------
# MHD   (quflow/integrators/mhd.py)
# -------------------------------------------------

def solve_mhd(state):
    """Hamiltonian of the standard MHD system, quflow/integrators/mhd.py:10-18:
    state = (W, Theta) -> (P, B) = (Delta^-1 W, Delta Theta), both on the device."""
    W = state[0, :, :]
    Theta = state[1, :, :]
    P = _laplacian.solve_poisson(W)
    B = _laplacian.laplace(Theta)
    return P, B


def magmp_fixedpoint(W, dt, steps=100, hamiltonian=solve_mhd, time=None, forcing=None, stats=None,
                     callback=None, tol='auto', maxit=10, minit=1, verbatim=False, reinitialize=False,
                     device=None):
    """Magnetic isospectral midpoint method for the MHD system
    W' = [P, W] + [B, Theta],  Theta' = [P, Theta]  (quflow/integrators/mhd.py:235-456);
    `W` is the (2,N,N) state (W, Theta), overwritten and returned.  All six products of an
    iteration, the Poisson solve, the Laplacian and the updates run on the device (qf_isomp_states
    with magnetic=1).  stats receives 'tol', 'iterations', 'maxit' like the reference (:341,452-454).
    """
    _check_iterations(minit, maxit)
    _refuse_stochastic(forcing, "magmp")
    if not isinstance(W, np.ndarray) or W.ndim != 3 or W.shape[0] != 2 or W.shape[1] != W.shape[2]:
        raise ValueError("the MHD state must be a (2,N,N) ndarray (W, Theta)")
    steps = _reference_args(W, steps)         # (mhd.py: `for k in range(steps)`, in-place updates of the state)
    if steps == 0 and not np.issubdtype(W.dtype, np.complexfloating):
        return W                 # the reference's empty loop never touches a real / integer W
    native_mhd = hamiltonian is solve_mhd or (getattr(hamiltonian, "__name__", "") == "solve_mhd" and
                                              (getattr(hamiltonian, "__module__", "") or "").startswith("quflow"))
    if forcing is not None or callback is not None or not native_mhd:
        # forcing(P, state[, time]), callback(state, 2 PWcomm), a foreign hamiltonian(state[, time]) -> (P, B)
        # (mhd.py:296-314, 395-402, 427-428): the hooked device loop in its magnetic mode
        return _magmp_hooked(W, dt, steps, hamiltonian, native_mhd, time, forcing, stats, callback, tol, maxit, minit,
                             verbatim, reinitialize, device)
    return _isomp_states(W, dt, steps, tol, minit, maxit, reinitialize, True, stats, verbatim, device,
                         tol_key='tol', maxit_key='maxit')


magmp = magmp_fixedpoint


# -------------------------------------------------
# OTHER ISOSPECTRAL METHODS   (quflow/integrators/isospectral.py:155-335)
# -------------------------------------------------

def _reference_args(W, steps):
    """What every stepper of the reference does with its state and step count before anything else happens: `range(steps)` (a
    float is a TypeError, a negative count an empty loop) and in-place complex updates of W (numpy refuses them for a real or
    integer array: UFuncTypeError, a TypeError).  Returns the step count to run."""
    if not isinstance(W, np.ndarray):
        raise TypeError("W must be a numpy ndarray")
    steps = operator.index(steps)
    if steps <= 0:
        return 0                 # an empty loop: no in-place update is ever attempted, W comes back as it is (any dtype)
    if not np.issubdtype(W.dtype, np.complexfloating):
        raise TypeError("Cannot cast ufunc 'add' output from dtype('complex128') to dtype('%s') with casting rule 'same_kind'" % W.dtype)
    return steps


def _check_device_stepper_args(W, hamiltonian, forcing):
    _refuse_stochastic(forcing, "isomp_simple / isomp_quasinewton")
    if forcing is not None:
        # the reference accepts `forcing` here and never uses it (`assert NotImplementedError(...)` asserts a truthy
        # object: isospectral.py:185-186, 283-284); same result, but say so
        import warnings
        warnings.warn("isomp_simple / isomp_quasinewton ignore `forcing` (as the reference does: "
                      "quflow/integrators/isospectral.py:185-186, 283-284)", stacklevel=3)
    if not isinstance(W, np.ndarray):
        raise TypeError("W must be a numpy ndarray")
    if W.ndim != 2 or W.shape[0] != W.shape[1]:
        raise ValueError("W must be a square matrix")


def _lu_needs_hook_table(hamiltonian, ham=None):
    """The plain entry points are the default case (built-in or installed Hamiltonian, skew-Hermitian flags on); a
    foreign Hamiltonian or select_skewherm(False) goes through the hooked ones, whose table carries the two flags."""
    if ham is not None:
        return False
    return (not _is_native_hamiltonian(hamiltonian)) or not (_SKEW_HERM_ and _laplacian._SKEW_HERM_)


def _lu_hook_table(N, hamiltonian):
    table = _HookTable(N, 1, True)
    if not _is_native_hamiltonian(hamiltonian):
        table.set_hamiltonian(hamiltonian, False)
    return table


def isomp_quasinewton(W, dt, steps=100, hamiltonian=_laplacian.solve_poisson, forcing=None,
                      tol="auto", maxit=10, verbatim=False, **kwargs):
    """Isospectral midpoint method with the quasi-Newton iteration of
    quflow/integrators/isospectral.py:155-251; W is overwritten and returned.  The two linear
    solves per iteration with A = I - (stepsize/2) Ptilde run on the matrix cores (Newton-Schulz
    inverse, include/quflow_hip.h) instead of LAPACK's LU: same iteration, same result to
    rounding.  `stats` (optional keyword) receives iterations / number_of_maxit / tol."""
    _check_device_stepper_args(W, hamiltonian, forcing)
    steps = _reference_args(W, steps)
    if steps == 0 and not np.issubdtype(W.dtype, np.complexfloating):
        return W                 # the reference's empty loop never touches a real / integer W
    tol_c = _tol_arg(tol)
    if tol_c < 0 and W.dtype == np.complex64:
        # isospectral.py:194-195 with the machine epsilon of the input's precision
        tol_c = float(np.finfo(np.float32).eps * (dt / hbar(W.shape[-1])) * np.linalg.norm(W, np.inf))
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    st = _lib.IsompStats()
    ham = _installable(hamiltonian, W)
    if not _lu_needs_hook_table(hamiltonian, ham):
        ctx = get_context(W.shape[-1], kwargs.get("device"))
        with _hamiltonian_on(ctx, ham):
            _lib.check(ctx._lib.qf_upload_W(ctx.handle, ptr(Wc)))
            _lib.check(ctx._lib.qf_isomp_quasinewton(ctx.handle, float(dt), int(steps), tol_c, int(maxit), ctypes.byref(st)))
        _lib.check(ctx._lib.qf_download_W(ctx.handle, ptr(Wc)))
    else:
        # a foreign Hamiltonian (isospectral.py:207): called back once per pass on host copies; the linear solves and
        # the update stay on the device.  A context of its own: the hook may use the shared one.  With
        # select_skewherm(False) the reference runs the very same formulas (its `assert NotImplementedError(...)`,
        # :188-189, asserts a truthy object) on the general branch of the Poisson solve.
        with _stepper_context(W.shape[-1], kwargs.get("device")) as ctx:
            table = _lu_hook_table(W.shape[-1], hamiltonian)
            _lib.check(ctx._lib.qf_upload_W(ctx.handle, ptr(Wc)))
            table.check(ctx._lib.qf_isomp_quasinewton_hooked(ctx.handle, float(dt), int(steps), tol_c, int(maxit),
                                                             ctypes.byref(st), ctypes.byref(table.c)))
            _lib.check(ctx._lib.qf_download_W(ctx.handle, ptr(Wc)))
    if Wc is not W:
        W[...] = Wc
    stats = kwargs.get("stats")
    _report_iterations(stats, verbatim, st, steps)
    if stats is not None and steps > 0:
        stats["tol"] = st.tol_used
    return W


def isomp_simple(W, dt, steps=100, hamiltonian=_laplacian.solve_poisson, forcing=None, **kwargs):
    """The simplified (explicit) isospectral midpoint method,
    quflow/integrators/isospectral.py:254-335; W is overwritten and returned."""
    _check_device_stepper_args(W, hamiltonian, forcing)
    steps = _reference_args(W, steps)
    if steps == 0 and not np.issubdtype(W.dtype, np.complexfloating):
        return W                 # the reference's empty loop never touches a real / integer W
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    ham = _installable(hamiltonian, W)
    if not _lu_needs_hook_table(hamiltonian, ham):
        ctx = get_context(W.shape[-1], kwargs.get("device"))
        with _hamiltonian_on(ctx, ham):
            _lib.check(ctx._lib.qf_upload_W(ctx.handle, ptr(Wc)))
            _lib.check(ctx._lib.qf_isomp_simple(ctx.handle, float(dt), int(steps)))
        _lib.check(ctx._lib.qf_download_W(ctx.handle, ptr(Wc)))
    else:
        # a foreign Hamiltonian (isospectral.py:286) and / or select_skewherm(False): the general branch (:303-314)
        with _stepper_context(W.shape[-1], kwargs.get("device")) as ctx:
            table = _lu_hook_table(W.shape[-1], hamiltonian)
            _lib.check(ctx._lib.qf_upload_W(ctx.handle, ptr(Wc)))
            table.check(ctx._lib.qf_isomp_simple_hooked(ctx.handle, float(dt), int(steps), ctypes.byref(table.c)))
            _lib.check(ctx._lib.qf_download_W(ctx.handle, ptr(Wc)))
    if Wc is not W:
        W[...] = Wc
    return W


# -------------------------------------------------
# CLASSICAL (EXPLICIT, NON-ISOSPECTRAL) INTEGRATORS   (quflow/integrators/erk.py)
# -------------------------------------------------

def update_stats(stats, **kwargs):
    """quflow/integrators/isospectral.py:85-90."""
    for arg, val in kwargs.items():
        if arg in stats and np.isscalar(val):
            stats[arg] += val
        else:
            stats[arg] = val


def _erk(method, W, dt, steps, hamiltonian, forcing, device=None):
    """euler / heun / rk4 on one (N,N) state or a (k,N,N) stack (P from state 0, bracket(P, W) broadcast over the stack:
    erk.py with (k,N,N) input).  With `forcing(P, W)` or a foreign `hamiltonian(W)` (erk.py:47-56, 93-112, 142-160) the
    hooked entry points keep the states and the stage combinations on the device and call back."""
    _refuse_stochastic(forcing, method)       # (noise inside Runge-Kutta stages is not defined here)
    steps = _reference_args(W, steps)         # (erk.py: `for k in range(steps)`, in-place updates of W)
    if steps == 0 and not np.issubdtype(W.dtype, np.complexfloating):
        return W                 # the reference's empty loop never touches a real / integer W
    # a TridiagonalHamiltonian without `forcing` is installed for the call (with `forcing` it is the foreign callable)
    ham = _installable(hamiltonian, W) if forcing is None and _laplacian._SKEW_HERM_ and W.ndim in (2, 3) else None
    stacked = W.ndim == 3 and W.shape[1] == W.shape[2]
    if not stacked and (W.ndim != 2 or W.shape[0] != W.shape[1]):
        raise ValueError("W must be a square matrix or a (k,N,N) stack")
    foreign = not (ham is not None or _is_native_hamiltonian(hamiltonian))
    hooked = forcing is not None or foreign
    if hooked and W.dtype != np.complex128:
        raise NotImplementedError("forcing / foreign Hamiltonians need a complex128 state on the HIP path.")
    N, k = W.shape[-1], (W.shape[0] if stacked else 1)
    Wc = np.ascontiguousarray(W, dtype=np.complex128)
    call = (_lib.ERK_METHODS[method], float(dt), int(steps))
    if hooked:
        # hooks see the whole stack; a foreign Hamiltonian returns one stream matrix for all states or one per state: the
        # first stage's evaluation tells.  An AffineForcing on one (N,N) state is installed on the device: no forcing hook
        table = _HookTable(N, k, not stacked)
        aff = _installable_forcing(forcing, W)
        if forcing is not None and aff is None:
            table.set_forcing(forcing, False)
        if not _is_native_hamiltonian(hamiltonian):
            table.set_hamiltonian(hamiltonian, False, per_state=(None if k > 1 else False))
        with _stepper_context(N, device) as ctx, _forcing_on(ctx, aff):
            if stacked:
                rc = ctx._lib.qf_erk_states_hooked(ctx.handle, ptr(Wc), int(k), *call, ctypes.byref(table.c))
            else:
                rc = ctx._lib.qf_erk_hooked(ctx.handle, ptr(Wc), *call, ctypes.byref(table.c))
        table.check(rc)
    else:
        ctx = get_context(N, device)
        with _hamiltonian_on(ctx, ham):
            if stacked:
                _lib.check(ctx._lib.qf_erk_states(ctx.handle, ptr(Wc), int(k), *call, int(_laplacian._SKEW_HERM_)))
            else:
                _lib.check(ctx._lib.qf_upload_W(ctx.handle, ptr(Wc)))
                _lib.check(ctx._lib.qf_erk(ctx.handle, *call, int(_laplacian._SKEW_HERM_)))
                _lib.check(ctx._lib.qf_download_W(ctx.handle, ptr(Wc)))
    if Wc is not W:
        W[...] = Wc                  # in-place contract (erk.py:56,110,156)
    return W


def euler(W, dt, steps=100, hamiltonian=_laplacian.solve_poisson, forcing=None, stats=None, **kwargs):
    """Euler's explicit first order method, quflow/integrators/erk.py:19-59; W is overwritten
    and returned.  The whole call (Poisson solves, products, updates) runs on the device; with
    `forcing` or a foreign Hamiltonian the hooks are called back from the device-resident loop."""
    W = _erk("euler", W, dt, steps, hamiltonian, forcing, kwargs.get("device"))
    if stats is not None:
        update_stats(stats, steps=steps)          # erk.py:58-59
    return W


def heun(W, dt, steps=100, hamiltonian=_laplacian.solve_poisson, forcing=None, device=None):
    """Heun's second order method, quflow/integrators/erk.py:62-112."""
    return _erk("heun", W, dt, steps, hamiltonian, forcing, device)


def rk4(W, dt, steps=100, hamiltonian=_laplacian.solve_poisson, forcing=None, device=None):
    """The classical Runge-Kutta fourth order method, quflow/integrators/erk.py:115-160."""
    return _erk("rk4", W, dt, steps, hamiltonian, forcing, device)


class IsompHIP:
    """`IsompHIP(N, dtype)` pre-creates the device context (buffers, factor tables, stream)
    like IsompCUDA.__init__ (quflow/experimental/isospectral_cuda.py:52-80); calling it
    has the stepper signature.  Unlike IsompCUDA it updates W in place AND returns it."""

    def __init__(self, N, dtype=np.complex128, device=None):
        self.N = int(N)
        self.dtype = np.dtype(dtype)
        self.device = device
        self.ctx = get_context(self.N, device)

    def __call__(self, W, dt, steps=100, hamiltonian=_laplacian.solve_poisson, time=None, forcing=None,
                 strang_splitting=None, stats=None, callback=None, tol='auto', maxit=10, minit=1,
                 verbatim=False, compsum=False, reinitialize=False):
        if W.shape[-1] != self.N:
            raise ValueError("IsompHIP was built for N=%d, got W of size %d" % (self.N, W.shape[-1]))
        return isomp_fixedpoint(W, dt, steps=steps, hamiltonian=hamiltonian, time=time, forcing=forcing,
                                strang_splitting=strang_splitting, stats=stats, callback=callback, tol=tol,
                                maxit=maxit, minit=minit, verbatim=verbatim, compsum=compsum,
                                reinitialize=reinitialize, device=self.device)


class DeviceTrajectory:
    """Keeps one trajectory resident in HBM across chunks (no PCIe traffic between
    `advance` calls); used by bench.py and the ensemble driver.  Each `advance` has the
    semantics of one `integrator(W, dt, steps=...)` call of simulation.solve
    (quflow/simulation.py:782-798): dW restarts from zero (isospectral.py:430)."""

    forcing = None              # (class defaults: _bare builds instances without __init__)
    strang_splitting = None
    hamiltonian = None

    @classmethod
    def _bare(cls, N, device=None, ctx=None):
        """A complex128 trajectory without a state of its own yet, on `ctx` or on a new private context: what from_shr / from_fun
        fill and what a DeviceStackTrajectory reaches its members through."""
        self = cls.__new__(cls)
        self.N, self.c64, self.dtype = int(N), False, np.complex128
        self.ctx = Context(self.N, default_device() if device is None else device) if ctx is None else ctx
        self._lib = self.ctx._lib
        self.hamiltonian = None
        return self

    def __init__(self, W0, device=None, hamiltonian=None, forcing=None, strang_splitting=None):
        """`hamiltonian`: None / solve_poisson for the built-in one, or a TridiagonalHamiltonian, which is installed on the
        trajectory's private context for its whole life: advance, advance_erk and advance_lu follow it.
        `forcing`: None, an AffineForcing or a StochasticForcing, installed for the trajectory's life (set_forcing replaces it
        between advances); a StochasticForcing starts at its counter `.step` and has it advanced by every `advance`;
        `strang_splitting`: None or a ViscDampStep, the viscous / damped half step around every step.  With either one
        `advance` is the hooked loop on the resident state (qf_isomp_forced: the bits of
        isomp(W, dt, steps, forcing=..., strang_splitting=...), nothing crosses PCIe); complex128 only."""
        # a complex64 initial state makes a single-precision trajectory (float32 solve, complex64 products:
        # what the reference does with complex64 input); anything else is complex128
        self.c64 = np.asarray(W0).dtype == np.complex64 and _laplacian.single_precision_on_device()
        self.dtype = np.complex64 if self.c64 else np.complex128
        W0 = np.ascontiguousarray(W0, dtype=self.dtype)
        self.N = W0.shape[-1]
        tridiagonal = isinstance(hamiltonian, _laplacian.TridiagonalHamiltonian)
        if tridiagonal:
            hamiltonian.check_size(self.N)
            if self.c64 or not (_laplacian.installable(hamiltonian) and _SKEW_HERM_):
                raise NotImplementedError("a resident TridiagonalHamiltonian needs complex128 data and the skew-Hermitian "
                                          "mode (select_skewherm(True))")
        elif not _is_native_hamiltonian(hamiltonian):
            raise TypeError("DeviceTrajectory takes the built-in Hamiltonian or a TridiagonalHamiltonian; any other callable "
                            "runs through isomp(..., hamiltonian=...)")
        if forcing is not None and not isinstance(forcing, _laplacian.DEVICE_FORCINGS):
            raise TypeError("DeviceTrajectory takes an AffineForcing or a StochasticForcing; any other callable runs through "
                            "isomp(..., forcing=...)")
        if strang_splitting is not None and not isinstance(strang_splitting, _laplacian.ViscDampStep):
            raise TypeError("DeviceTrajectory takes a ViscDampStep; any other callable runs through "
                            "isomp(..., strang_splitting=...)")
        if forcing is not None or strang_splitting is not None:
            if self.c64 or not (_SKEW_HERM_ and _laplacian._SKEW_HERM_):
                raise NotImplementedError("a resident forcing / strang_splitting needs complex128 data and the "
                                          "skew-Hermitian mode (select_skewherm(True))")
            if forcing is not None:
                forcing.check_size(self.N)
        # a private context: the trajectory owns its device state (the shared per-N context of
        # get_context() is scratch for the host-in/host-out entry points)
        self.ctx = Context(self.N, default_device() if device is None else device)
        self._lib = self.ctx._lib
        self.hamiltonian = None
        if tridiagonal:
            try:
                hamiltonian.install(self.ctx)
            except Exception:
                self.ctx.close()
                raise
            self.hamiltonian = hamiltonian
        self.strang_splitting = strang_splitting
        try:
            self.set_forcing(forcing)
        except Exception:
            self.ctx.close()
            raise
        _lib.check((self._lib.qf_c64_upload_W if self.c64 else self._lib.qf_upload_W)(self.ctx.handle, ptr(W0)))

    def set_forcing(self, forcing):
        """Replace the installed forcing between advances (None: none): an AffineForcing, or a StochasticForcing, whose
        pattern is redrawn on the device for every step from its counter `.step` on."""
        if forcing is None:
            if self.forcing is not None:
                _laplacian.AffineForcing.uninstall(self.ctx)
            self.forcing = None
            return
        if not isinstance(forcing, _laplacian.DEVICE_FORCINGS):
            raise TypeError("DeviceTrajectory takes an AffineForcing or a StochasticForcing; any other callable runs through "
                            "isomp(..., forcing=...)")
        if self.c64 or not (_SKEW_HERM_ and _laplacian._SKEW_HERM_):
            raise NotImplementedError("a resident forcing needs complex128 data and the skew-Hermitian mode "
                                      "(select_skewherm(True))")
        forcing.check_size(self.N)
        forcing.install(self.ctx)
        self.forcing = forcing

    def _stochastic(self, what):
        if not isinstance(self.forcing, _laplacian.StochasticForcing):
            raise ValueError("%s: no StochasticForcing is installed on this trajectory" % what)
        return self.forcing

    def stochastic_tell(self):
        """The counter of the next step's noise, read from the device context (qf_stochastic_tell)."""
        return self._stochastic("stochastic_tell").sync(self.ctx)

    def stochastic_seek(self, step):
        """Set the counter of the next step's noise (qf_stochastic_seek); the installed forcing's `.step` follows."""
        f = self._stochastic("stochastic_seek")
        step = _laplacian._uint64_arg("step", step)
        _lib.check(self._lib.qf_stochastic_seek(self.ctx.handle, ctypes.c_ulonglong(step)))
        f.step = step

    def hamiltonian_energy(self):
        """H = -inner_L2(P, W - F)/2 of the resident state with P = T^-1 (W - F) of the installed Hamiltonian (the built-in
        one: energy_euler): the conserved energy of the flow when T is symmetric.  `diagnostics()` keeps reporting
        energy_euler, the built-in Poisson energy, whatever is installed."""
        self._double_only("hamiltonian_energy")
        e = ctypes.c_double()
        _lib.check(self._lib.qf_hamiltonian_energy(self.ctx.handle, ctypes.byref(e)))
        return e.value

    def advance(self, dt, steps, tol='auto', maxit=10, minit=1, compsum=False, reinitialize=False, diagnostics=False):
        """`diagnostics=True`: energy_euler and enstrophy of the new state come back with the statistics
        (keys "energy", "enstrophy"), computed behind the last step under the call's one synchronisation
        (qf_isomp_diag) -- what an output chunk of simulation.solve logs (quflow/simulation.py:788-803)."""
        _check_iterations(minit, maxit)
        tol_c = -1.0 if isinstance(tol, str) else float(tol)
        st = _lib.IsompStats()
        args = (self.ctx.handle, float(dt), int(steps), tol_c, int(minit), int(maxit), int(bool(compsum)),
                int(bool(reinitialize)), ctypes.byref(st))
        out = {}
        if self.forcing is not None or self.strang_splitting is not None:
            # the hooked loop on the resident state, with what is installed (qf_isomp_forced)
            if compsum and self.forcing is not None:
                raise NotImplementedError("Compensated sum with forcing is not yet implemented.")     # isospectral.py:588-589
            if compsum:
                raise NotImplementedError("compsum with a resident strang_splitting: run it through "
                                          "isomp(..., strang_splitting=..., compsum=True)")
            tab, key = (None, 0)
            if self.strang_splitting is not None:
                tab, key = self.strang_splitting.table_and_key(self.N, dt / 2)
                tab = np.ascontiguousarray(tab, dtype=np.float64)
            try:
                _lib.check(self._lib.qf_isomp_forced(self.ctx.handle, float(dt), int(steps), tol_c, int(minit), int(maxit),
                                                     int(bool(reinitialize)), None if tab is None else ptr(tab),
                                                     ctypes.c_ulonglong(key), ctypes.byref(st)))
            finally:
                if isinstance(self.forcing, _laplacian.StochasticForcing):
                    self.forcing.sync(self.ctx)        # the counter the call left
            if diagnostics:
                e, s = self.diagnostics()
                out = {"energy": e, "enstrophy": s}
        elif self.c64:
            _lib.check(self._lib.qf_c64_isomp(*args))
            if diagnostics:
                e, s = self.diagnostics()
                out = {"energy": e, "enstrophy": s}
        elif diagnostics:
            e = ctypes.c_double()
            s = ctypes.c_double()
            _lib.check(self._lib.qf_isomp_diag(*args, ctypes.byref(e), ctypes.byref(s)))
            out = {"energy": e.value, "enstrophy": s.value}
        else:
            _lib.check(self._lib.qf_isomp(*args))
        out.update(_stats_dict(st, steps))
        return out

    def advance_erk(self, method, dt, steps):
        """`steps` steps of euler / heun / rk4 (quflow/integrators/erk.py) on the resident state."""
        self._double_only("advance_erk")
        self._unforced_only("advance_erk")
        _lib.check(self._lib.qf_erk(self.ctx.handle, _lib.ERK_METHODS[method], float(dt), int(steps),
                                    int(_laplacian._SKEW_HERM_)))
        evals = {"euler": 1, "heun": 2, "rk4": 4}[method]
        return {"iterations": float(evals), "number_of_maxit": 0.0, "total_iterations": evals * int(steps),
                "tol": 0.0, "last_resnorm": 0.0}

    def advance_lu(self, method, dt, steps, tol=-1.0, maxit=10):
        """`steps` steps of isomp_simple / isomp_quasinewton (isospectral.py:155-335) on the resident state."""
        self._double_only("advance_lu")
        self._unforced_only("advance_lu")
        st = _lib.IsompStats()
        if method == "isomp_simple":
            _lib.check(self._lib.qf_isomp_simple(self.ctx.handle, float(dt), int(steps)))
            st.total_iterations = int(steps)
        else:
            _lib.check(self._lib.qf_isomp_quasinewton(self.ctx.handle, float(dt), int(steps), float(tol), int(maxit),
                                                      ctypes.byref(st)))
        return _stats_dict(st, steps)

    def _double_only(self, what):
        if self.c64:
            raise NotImplementedError("%s on a complex64 trajectory: the resident single-precision state has the "
                                      "stepper (advance), diagnostics, upload and download; convert to complex128 "
                                      "for the rest" % what)

    def _unforced_only(self, what):
        if self.forcing is not None:
            raise NotImplementedError("%s with an installed forcing: the resident forced run has the isomp stepper "
                                      "(advance); euler / heun / rk4 take forcing= on host arrays" % what)

    def diagnostics(self):
        """(energy_euler, enstrophy) of the resident state, quflow/physics.py:26-38."""
        e = ctypes.c_double()
        s = ctypes.c_double()
        fn = self._lib.qf_c64_diagnostics if self.c64 else self._lib.qf_diagnostics
        _lib.check(fn(self.ctx.handle, ctypes.byref(e), ctypes.byref(s)))
        return e.value, s.value

    def casimirs(self, kmax=4):
        """C_k = Re tr((iW)^k) / N, k = 1..kmax <= 8, of the resident state: the (kmax,) array quflow_amd.physics.casimirs
        gives for `download()`, without the download (qf_casimirs; a complex64 state is widened on the device and summed in
        double, qf_c64_casimirs).  At most three products and one reduction pass, cheap enough to log per chunk.  The state,
        the carried increment and the statistics of the run are untouched: the next `advance` continues bit for bit as if
        the call had not happened."""
        from .physics import casimirs_call, check_kmax
        kmax = check_kmax(kmax)
        if self.c64:
            return casimirs_call(self._lib.qf_c64_casimirs, kmax, self.ctx.handle)
        return casimirs_call(self._lib.qf_casimirs, kmax, self.ctx.handle, None)

    def _need_basis(self):
        """The transforms' mode on this trajectory's context, by quantization.use_streamed: above the resident limit
        (N > 2048 by default) the blocks are rebuilt slab by slab for each call, else the basis is computed once."""
        from .quantization import use_streamed, slab_bytes
        if use_streamed(self.N):
            _lib.check(self._lib.qf_basis_stream(self.ctx.handle, ctypes.c_longlong(slab_bytes())))
            return
        if not getattr(self, "_basis_ready", False):
            _lib.check(self._lib.qf_basis_compute(self.ctx.handle))     # quantization.py:68-113, on the device
            self._basis_ready = True
        _lib.check(self._lib.qf_basis_stream(self.ctx.handle, ctypes.c_longlong(0)))

    @classmethod
    def from_shr(cls, omega, N=-1, device=None):
        """Start a trajectory from real spherical-harmonics coefficients: W0 = shr2mat(omega, N)
        (quflow/quantization.py:450-489) is built straight into the resident state."""
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        if N == -1:
            N = round(np.sqrt(omega.shape[0]))
        self = cls._bare(N, device)
        self._need_basis()
        _lib.check(self._lib.qf_shr2mat(self.ctx.handle, ptr(omega), ctypes.c_longlong(omega.shape[0]), None))
        return self

    @classmethod
    def from_fun(cls, f, N=-1, device=None):
        """Start a trajectory from a real function on the MW grid (L, 2L-1): W0 = shr2mat(sht.fun2shr(f), N) built
        straight into the resident state.  Only the grid crosses PCIe: the analysis leaves its L^2 coefficients on the
        device, where shr2mat reads them.  N = -1 means N = L; L < N band-limits as shr2mat does for a short omega; L > N
        is refused.  The trajectory is then the one from_shr(sht.fun2shr(f), N) gives, bit for bit."""
        from .sht import _grid
        f, L, isreal = _grid(f)
        assert isreal, "f must be a real array."
        if N == -1:
            N = L
        N = int(N)
        if L > N:
            raise ValueError("from_fun: the grid's bandwidth L=%d exceeds the matrix size N=%d" % (L, N))
        self = cls._bare(N, device)
        self._need_basis()
        _lib.check(self._lib.qf_fun2shr(self.ctx.handle, ptr(f), L, 1, None))
        _lib.check(self._lib.qf_shr2mat(self.ctx.handle, None, ctypes.c_longlong(L * L), None))
        return self

    def shr(self, n_omega=None):
        """mat2shr of the resident state (quflow/quantization.py:492-525): what simulation.py:287-344
        stores for an 'shr' output -- N^2 doubles cross PCIe instead of the N^2 complex state."""
        self._double_only("shr")
        self._need_basis()
        n = self.N * self.N if n_omega is None else int(n_omega)
        omega = np.zeros(n, dtype=np.float64)
        _lib.check(self._lib.qf_mat2shr(self.ctx.handle, None, ptr(omega), ctypes.c_longlong(n)))
        return omega

    def fun(self, n_omega=None, berezin=True):
        """shr2fun(self.shr(n_omega), berezin=berezin) (quflow/transforms.py:422-438) with the coefficients kept on the
        device: only the (L, 2L-1) grid crosses PCIe, L = sqrt(n_omega).  n_omega = (N//2)**2 is the reference's 'funhalf'
        output, berezin=False its 'funL2' (simulation.py:287-344)."""
        from .transforms import _bandwidth
        self._double_only("fun")
        self._need_basis()
        n = self.N * self.N if n_omega is None else int(n_omega)
        L = _bandwidth(n, -1)
        f = np.empty((L, 2 * L - 1), dtype=np.float64)
        _lib.check(self._lib.qf_mat2shr(self.ctx.handle, None, None, ctypes.c_longlong(n)))
        _lib.check(self._lib.qf_shr2fun(self.ctx.handle, None, ctypes.c_longlong(n), L, int(bool(berezin)), ptr(f)))
        return f

    def fields(self, qutypes):
        """The function-space outputs of the resident state, {qutype: array}: `qutypes` is a dict in the reference's form
        restricted to 'fun', 'funL2', 'funhalf', 'funL2half' with dtypes float32 / float64 (simulation.py:313-342).  Each
        grid is `self.fun(n_omega, berezin).astype(dtype)` bit for bit ('half': n_omega = (N//2)**2, 'L2': berezin=False),
        but the state goes through mat2shr once, the fields of one bandwidth share one synthesis and the cast happens on
        the device (qf_state_fields): a float32 grid crosses PCIe as float32.  The state, the carried increment and the
        statistics of the run are untouched: the next `advance` continues bit for bit as if the call had not happened."""
        from .transforms import _fields_call
        self._double_only("fields")
        self._need_basis()
        return _fields_call(self.ctx, None, self.N, qutypes)

    def fields_and_shr(self, qutypes):
        """(self.fields(qutypes), self.shr()), bit for bit, for a record that stores both: when the sweep that made the
        fields has left mat2shr of the whole state on the device (a field of the full bandwidth with a resident basis, or
        swept last with a streamed one) the coefficients are copied out (qf_shr_held) instead of swept again.  The library
        decides: QF_ERR_STATE from qf_shr_held means the device copy holds fewer coefficients, and `shr()` sweeps."""
        out = self.fields(qutypes)
        omega = np.zeros(self.N * self.N, dtype=np.float64)
        rc = self._lib.qf_shr_held(self.ctx.handle, ptr(omega), ctypes.c_longlong(omega.shape[0]))
        if rc == 4:                       # QF_ERR_STATE
            return out, self.shr()
        _lib.check(rc)
        return out, omega

    def spectral_budget(self, lmax=None, coefficients=False):
        """quflow_amd.analysis.spectral_budget of the resident state with what is installed on this trajectory -- its
        Hamiltonian, its forcing (of a StochasticForcing only the affine terms a_W, a_P, a_lap: the noise pattern belongs
        to a step and does not enter, the counter is not touched), the dissipation of its ViscDampStep -- from one sweep of
        the basis; 3 lmax doubles cross PCIe (and the coefficients when asked).  The state, the carried increment and the
        statistics of the run are untouched: the next `advance` continues bit for bit as if the call had not happened."""
        from . import analysis
        self._double_only("spectral_budget")
        nmax = analysis._band_limit(self.N, lmax)
        analysis._check_budget_mode("spectral_budget")
        self._need_basis()
        return analysis._budget_call(self.ctx, None, nmax, self.forcing is not None, self.strang_splitting, coefficients)

    def _degree_spectrum(self, what):
        from . import analysis
        self._double_only(what)
        self._need_basis()
        return np.arange(1, self.N), analysis._spectrum_call(self.ctx, None, self.N)[1:]

    def enstrophy_spectrum(self):
        """(el, enstrophy) of the resident state as quflow_amd.analysis.enstrophy_spectrum gives it, summed per degree on
        the device (qf_degree_spectrum: no solve, no product): N doubles cross PCIe instead of the N^2 of `shr()`."""
        return self._degree_spectrum("enstrophy_spectrum")

    def energy_spectrum(self, beta=0):
        """(el, energy) of the resident state as quflow_amd.analysis.energy_spectrum gives it, from the same sums."""
        el, Z = self._degree_spectrum("energy_spectrum")
        return el, Z / (el * (el + 1)) ** (1 - beta / 2)

    def spectrum(self):
        """The ascending eigenvalues of -i W for the resident state: the invariant of the isospectral flow, by the
        device eigensolver (qf_eigh_state, quflow_amd.linalg).  Only the N eigenvalues cross PCIe."""
        self._double_only("spectrum")
        lam = np.empty(self.N, dtype=np.float64)
        _lib.check_eigh(self._lib.qf_eigh_state(self.ctx.handle, ptr(lam), None))
        return lam

    def scale_decomposition(self):
        """Host (Ws, Wr) of the resident state with P = solve_poisson(W): quflow_amd.analysis.scale_decomposition of
        `download()`, without the download."""
        self._double_only("scale_decomposition")
        Ws = np.empty((self.N, self.N), dtype=np.complex128)
        Wr = np.empty((self.N, self.N), dtype=np.complex128)
        _lib.check_eigh(self._lib.qf_scale_decomposition(self.ctx.handle, None, None, ptr(Ws), ptr(Wr)))
        return Ws, Wr

    def rotate(self, xi):
        """Rotate the resident state in place, W <- R W R^H with R = exp(xi . S) (quflow_amd.geometry.rotate of
        `download()`, bit for bit, without any transfer).  The next `advance` starts as after an `upload`.  Returns self."""
        self._double_only("rotate")
        xi = np.ascontiguousarray(xi, dtype=np.float64)
        if xi.shape != (3,):
            raise ValueError("xi must have shape (3,), got %s" % (xi.shape,))
        _lib.check_eigh(self._lib.qf_rotate(self.ctx.handle, xi.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None))
        return self

    def grad(self):
        """(3,N,N) host array: quflow_amd.geometry.grad of the resident state, without the upload."""
        self._double_only("grad")
        dP = np.empty((3, self.N, self.N), dtype=np.complex128)
        _lib.check_eigh(self._lib.qf_grad(self.ctx.handle, None, ptr(dP)))
        return dP

    def download(self):
        W = np.zeros((self.N, self.N), dtype=self.dtype)
        _lib.check((self._lib.qf_c64_download_W if self.c64 else self._lib.qf_download_W)(self.ctx.handle, ptr(W)))
        return W

    def upload(self, W):
        """Replace the resident state (e.g. after a call that ended in an error left it undefined)."""
        W = np.ascontiguousarray(W, dtype=self.dtype)
        if W.shape != (self.N, self.N):
            raise ValueError("state must be (%d, %d), got %s" % (self.N, self.N, W.shape))
        _lib.check((self._lib.qf_c64_upload_W if self.c64 else self._lib.qf_upload_W)(self.ctx.handle, ptr(W)))

    def sync(self):
        _lib.check(self._lib.qf_sync(self.ctx.handle))


MHD_KEYS = ("energy_kinetic", "energy_magnetic", "cross_helicity", "magnetic_casimir", "enstrophy")


def _mhd_dict(out):
    """qf_mhd_diagnostics' five values by name; `energy` = Ek + Em is the conserved Hamiltonian."""
    d = dict(zip(MHD_KEYS, (float(v) for v in out)))
    d["energy"] = d["energy_kinetic"] + d["energy_magnetic"]
    return d


def _check_stack(states, magnetic, N=None):
    """The (k,N,N) complex128 stack a resident stack trajectory takes, C-contiguous; ValueError otherwise."""
    states = np.asarray(states)
    if states.ndim != 3:
        raise ValueError("a stack of states must be a (k,N,N) array, got shape %s" % (states.shape,))
    if states.shape[0] < 1 or states.shape[1] != states.shape[2]:
        raise ValueError("the members of a stack must be square matrices, got shape %s" % (states.shape,))
    if states.dtype != np.complex128:
        raise ValueError("a resident stack is complex128, got %s" % states.dtype)
    if magnetic and states.shape[0] != 2:
        raise ValueError("the MHD state must be a (2,N,N) array (W, Theta), got shape %s" % (states.shape,))
    if N is not None and states.shape[-1] != N:
        raise ValueError("state must be (k, %d, %d), got %s" % (N, N, states.shape))
    return np.ascontiguousarray(states)


class DeviceStackTrajectory:
    """Keeps a (k,N,N) stack resident in HBM across chunks: what DeviceTrajectory is to one state.  Each `advance` has
    the semantics, and the bits, of one `isomp(stack, dt, steps=...)` call (state 0 drives the flow, the others are carried
    along; isospectral.py:463-611 on a 3-D W) or, with `magnetic=True` on the pair (W, Theta), of one
    `magmp(state, dt, steps=...)` call (mhd.py:235-456 with hamiltonian = solve_mhd): dX restarts from zero per call.
    Skew-Hermitian mode, complex128, the built-in Hamiltonian."""

    def __init__(self, states0, magnetic=False, device=None):
        states0 = _check_stack(states0, magnetic)
        if not (_SKEW_HERM_ and _laplacian._SKEW_HERM_):
            raise NotImplementedError("a resident stack needs the skew-Hermitian mode (select_skewherm(True))")
        self.magnetic = bool(magnetic)
        self.k, self.N = states0.shape[0], states0.shape[-1]
        self.dtype = np.complex128
        # a private context: the trajectory owns its device state (as DeviceTrajectory)
        self.ctx = Context(self.N, default_device() if device is None else device)
        self._lib = self.ctx._lib
        # member access: a DeviceTrajectory's resident helpers on this context's state W, where qf_states_select puts member j
        self._member = DeviceTrajectory._bare(self.N, ctx=self.ctx)
        try:
            _lib.check(self._lib.qf_states_upload(self.ctx.handle, ptr(states0), self.k))
        except Exception:
            self.ctx.close()
            raise

    def advance(self, dt, steps, tol='auto', maxit=10, minit=1, reinitialize=False, diagnostics=False):
        """The keys of DeviceTrajectory.advance; `diagnostics=True` adds `diagnostics()` of the new state -- for MHD queued
        behind the last step under the call's closing synchronisation (qf_states_advance_diag)."""
        _check_iterations(minit, maxit)
        tol_c = -1.0 if isinstance(tol, str) else float(tol)
        st = _lib.IsompStats()
        args = (self.ctx.handle, float(dt), int(steps), tol_c, int(minit), int(maxit), int(bool(reinitialize)),
                int(self.magnetic), ctypes.byref(st))
        out = {}
        if diagnostics and self.magnetic:
            d = (ctypes.c_double * 5)()
            _lib.check(self._lib.qf_states_advance_diag(*args, d))
            out = _mhd_dict(d)
        else:
            _lib.check(self._lib.qf_states_advance(*args))
            if diagnostics:
                out = self.diagnostics()
        out.update(_stats_dict(st, steps))
        return out

    def diagnostics(self):
        """MHD: energy_kinetic = -<W, Delta^-1 W>/2, energy_magnetic = -<Theta, Delta Theta>/2, energy (their sum, the
        conserved Hamiltonian), cross_helicity = <W, Theta>, magnetic_casimir = <Theta, Theta>/2, enstrophy = <W, W>/2 --
        one solve and one reduction pass on the device (qf_mhd_diagnostics).
        A stack of tracers: energy and enstrophy of state 0 and `members`, one (<X_j, X_0>, <X_j, X_j>/2) per member."""
        if self.magnetic:
            d = (ctypes.c_double * 5)()
            _lib.check(self._lib.qf_mhd_diagnostics(self.ctx.handle, d))
            return _mhd_dict(d)
        _lib.check(self._lib.qf_states_select(self.ctx.handle, 0))
        e, s = self._member.diagnostics()
        m = (ctypes.c_double * (2 * self.k))()
        _lib.check(self._lib.qf_states_inner(self.ctx.handle, m))
        return {"energy": e, "enstrophy": s, "members": [(m[2 * j], m[2 * j + 1]) for j in range(self.k)]}

    def casimirs(self, j, kmax=4):
        """DeviceTrajectory.casimirs of member j, read in place (qf_states_casimirs): the context's state W is not used."""
        from .physics import casimirs_call, check_kmax
        kmax = check_kmax(kmax)
        return casimirs_call(self._lib.qf_states_casimirs, kmax, self.ctx.handle, int(j))

    def mhd_casimirs(self, kmax=4):
        """What magmp conserves besides the energy, of the resident pair (W, Theta) (qf_mhd_casimirs):
        {"magnetic": C_k(Theta) for k = 1..kmax, "cross": Re tr((iW)(iTheta)^k) / N for k = 1..ceil(kmax / 2)}.
        magnetic[1] = 2 magnetic_casimir and cross[0] = cross_helicity of `diagnostics()`.  The run is untouched."""
        from .physics import check_kmax
        kmax = check_kmax(kmax)
        if not self.magnetic or self.k != 2:
            raise ValueError("mhd_casimirs are those of the MHD pair (W, Theta): this stack is not magnetic (k=%d)" % self.k)
        mag = np.empty(kmax, dtype=np.float64)
        cross = np.empty((kmax + 1) // 2, dtype=np.float64)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(self._lib.qf_mhd_casimirs(self.ctx.handle, kmax, mag.ctypes.data_as(dp), cross.ctypes.data_as(dp)))
        return {"magnetic": mag, "cross": cross}

    def _select(self, j):
        _lib.check(self._lib.qf_states_select(self.ctx.handle, int(j)))
        return self._member

    def shr(self, j, n_omega=None):
        """DeviceTrajectory.shr of member j."""
        return self._select(j).shr(n_omega)

    def fun(self, j, n_omega=None, berezin=True):
        """DeviceTrajectory.fun of member j."""
        return self._select(j).fun(n_omega, berezin)

    def fields(self, j, qutypes):
        """DeviceTrajectory.fields of member j."""
        return self._select(j).fields(qutypes)

    def spectral_budget(self, j, lmax=None, coefficients=False):
        """DeviceTrajectory.spectral_budget of member j (the built-in Hamiltonian, no forcing)."""
        return self._select(j).spectral_budget(lmax, coefficients)

    def mhd_budget(self, lmax=None, coefficients=False):
        """quflow_amd.analysis.mhd_spectral_budget of the resident pair (W, Theta) -- spectra of the kinetic and magnetic
        energy, the mean-square potential and the cross helicity, their transfers and fluxes per degree -- from one sweep of
        the basis; 9 lmax doubles cross PCIe (and the coefficients when asked).  The stack and the statistics of the run are
        untouched: the next `advance` continues bit for bit as if the call had not happened.  `spectral_budget(j)` remains
        the hydrodynamic budget of one member taken alone."""
        from . import analysis
        if not self.magnetic or self.k != 2:
            raise ValueError("mhd_budget is the budget of the MHD pair (W, Theta): this stack is not magnetic (k=%d)" % self.k)
        nmax = analysis._band_limit(self.N, lmax)
        analysis._check_budget_mode("mhd_budget")
        self._member._need_basis()
        return analysis._mhd_budget_call(self.ctx, nmax, coefficients)

    def spectrum(self, j):
        """DeviceTrajectory.spectrum of member j: the invariant of the flow for every member of the stack."""
        return self._select(j).spectrum()

    def rotate(self, xi):
        """Rotate every member in place, X_j <- R X_j R^H with R = exp(xi . S) (quflow_amd.geometry.rotate of each
        downloaded member, bit for bit, without any transfer).  Returns self."""
        for j in range(self.k):
            self._select(j).rotate(xi)
            _lib.check(self._lib.qf_states_store(self.ctx.handle, j))
        return self

    def download(self):
        states = np.zeros((self.k, self.N, self.N), dtype=np.complex128)
        _lib.check(self._lib.qf_states_download(self.ctx.handle, ptr(states), self.k))
        return states

    def upload(self, states):
        """Replace the resident stack (e.g. after a call that ended in an error)."""
        states = _check_stack(states, self.magnetic, self.N)
        if states.shape[0] != self.k:
            raise ValueError("state must be (%d, %d, %d), got %s" % (self.k, self.N, self.N, states.shape))
        _lib.check(self._lib.qf_states_upload(self.ctx.handle, ptr(states), self.k))

    def sync(self):
        _lib.check(self._lib.qf_sync(self.ctx.handle))


class DeviceMHDTrajectory(DeviceStackTrajectory):
    """The MHD pair (W, Theta) resident on the device: DeviceStackTrajectory(state0, magnetic=True)."""

    def __init__(self, state0, device=None):
        super().__init__(state0, magnetic=True, device=device)


class DeviceEnsemble:
    """k independent trajectories resident on ONE GPU, advanced together (qf_isomp_multi): each
    member is a DeviceTrajectory of its own -- own Hamiltonian, own exit decisions, own statistics,
    results bit-identical to advancing it alone -- but one host loop feeds all their streams, so the
    GPU overlaps the replicas.  For ensembles with more seeds than GPUs (quflow_amd.ensemble)."""

    def __init__(self, W0s, device=None, hamiltonian=None):
        self.members = [DeviceTrajectory(W0, device=device, hamiltonian=hamiltonian) for W0 in W0s]
        if not self.members:
            raise ValueError("DeviceEnsemble needs at least one initial condition")
        if len({m.N for m in self.members}) != 1:
            raise ValueError("the members of a DeviceEnsemble share one matrix size")
        if len({m.c64 for m in self.members}) != 1:
            raise ValueError("the members of a DeviceEnsemble share one dtype (complex128 or complex64)")
        self.c64 = self.members[0].c64
        self._lib = self.members[0]._lib

    def __len__(self):
        return len(self.members)

    # Members advanced at the same time: one per hardware pipe.  A stream's hardware queue number mod 4 is its pipe and two
    # replicas on one pipe lose 40 % of their combined rate (profiles/r06_x4_hardware_queues.txt: N = 512
    # sum 18,100 timesteps/s with four replicas, 13,000 with five, 16,100 with eight), so a larger ensemble goes through a
    # call in groups of four neighbours (created back to back: consecutive queues, four pipes).
    CONCURRENT = 4

    def advance(self, dt, steps, tol='auto', maxit=10, minit=1):
        """`steps` steps of every member (the semantics of one `integrator(W, dt, steps=...)` call each);
        returns one stats dict per member.

        A member whose residual turns inf / NaN (what raises in the reference's exit test) does not stop the others: every
        group of members is advanced, every member runs to its end, and then ONE ValueError is raised.  Its `failed`
        attribute lists the indices of the failed members, its `stats` attribute the per-member stats dicts (a failed
        member's is {"failed": True, "tol": ...}).  A failed member holds the state its own DeviceTrajectory.advance would
        leave on that failure (after its last completed step); every other member has advanced all `steps` steps, exactly
        as alone.  Any other error raises at once."""
        _check_iterations(minit, maxit)
        tol_c = -1.0 if isinstance(tol, str) else float(tol)
        for m in self.members:
            _refuse_stochastic(m.forcing, "DeviceEnsemble.advance")
        fn = self._lib.qf_c64_isomp_multi if self.c64 else self._lib.qf_isomp_multi
        out = []
        failed = []
        for g0 in range(0, len(self.members), self.CONCURRENT):
            group = self.members[g0:g0 + self.CONCURRENT]
            k = len(group)
            handles = (ctypes.c_void_p * k)(*[m.ctx.handle for m in group])
            st = (_lib.IsompStats * k)()
            rc = fn(handles, k, float(dt), int(steps), tol_c, int(minit), int(maxit), st)
            if rc != _lib.QF_ERR_NONFINITE:
                _lib.check(rc)
            for r, s in enumerate(st):
                # (qf_isomp_multi: a member whose call failed reports total_iterations = -1)
                if rc == _lib.QF_ERR_NONFINITE and s.total_iterations < 0:
                    failed.append(g0 + r)
                    out.append({"failed": True, "tol": s.tol_used})
                    continue
                out.append(_stats_dict(s, steps))
        if failed:
            err = ValueError("array must not contain infs or NaNs (DeviceEnsemble members %s)" % ", ".join(map(str, failed)))
            err.failed = failed
            err.stats = out
            raise err
        return out

    def diagnostics(self):
        return [m.diagnostics() for m in self.members]

    def casimirs(self, kmax=4):
        """(members, kmax) array: DeviceTrajectory.casimirs of every member, member by member as `diagnostics()`."""
        from .physics import check_kmax
        kmax = check_kmax(kmax)
        return np.stack([m.casimirs(kmax) for m in self.members])

    def download(self):
        return [m.download() for m in self.members]

    def sync(self):
        for m in self.members:
            m.sync()

    def close(self):
        for m in self.members:
            m.ctx.close()
