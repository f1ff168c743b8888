"""Laplacian backend module protocol of quflow, on the MI355X.

Mirrors `quflow.laplacian` (default backend quflow/laplacian/cpu.py re-exported by
quflow/laplacian/__init__.py:1): an object with `solve_poisson(W)`, `laplace(P)`,
`laplacian(N, bc)`, `select_skewherm(flag)` and `__name__` -- the interface the
reference's tests parametrise over (tests/test_laplacian.py:134-152,226-252).
Everything below runs hand-written HIP kernels through the C ABI
(include/quflow_hip.h); there is no CPU path.
"""
import collections
import ctypes
import hashlib

import numpy as np

from . import _lib
from . import geometry as _geometry
from .context import as_c128, get_context, ptr, result_array

_SKEW_HERM_ = True
_out_cache = {}


def select_skewherm(flag):
    """quflow/laplacian/cpu.py:563-591: returns the previous flag."""
    global _SKEW_HERM_
    old = _SKEW_HERM_
    _SKEW_HERM_ = bool(flag)
    return old


def select_first(W):
    """quflow/laplacian/cpu.py:672-674: state 0 of a (..., N, N) stack, contiguous -- the default `reduce` of
    solve_poisson (:681, 696-697)."""
    return np.ascontiguousarray(W[(0,) * (W.ndim - 2) + (Ellipsis,)])


def select_sum(W):
    """quflow/laplacian/cpu.py:677-678: the sum of the states -- `reduce=select_sum` makes every state of a stack a
    source of the one stream matrix."""
    return W.sum(axis=tuple(range(W.ndim - 2)))


_reduce_first = select_first


def allocate_buffer(W):
    """quflow/laplacian/cpu.py:594-601 warms the solver's per-N buffers for W's size and dtype.  Here: the device
    context of that size (tables, factors, device buffers) and the persistent result array of solve_poisson."""
    W = np.asarray(W)
    N = W.shape[0]
    get_context(N)
    _out_buffer(N, np.complex64 if W.dtype == np.complex64 else np.complex128)


def _out_buffer(N, dtype):
    """solve_poisson returns the SAME ndarray on every call (cpu.py:24-32,726,734)."""
    key = (N, np.dtype(dtype).str)
    if key not in _out_cache:
        _out_cache[key] = np.zeros((N, N), dtype=dtype)
    return _out_cache[key]


def single_precision_on_device():
    """complex64 data is computed in float32 on the device, as the reference computes it (float32 tables and
    solve, cpu.py:725; complex64 products).  QUFLOW_HIP_C64=f64 restores the double-precision evaluation with a
    cast of the result (A/B runs)."""
    import os
    return os.environ.get("QUFLOW_HIP_C64", "f32") != "f64"


def laplacian(N, bc=False, dtype=np.float64):
    """Coefficient table (N,N,2) of the quantized Laplacian, quflow/laplacian/cpu.py:55-95,604-625.
    dtype=float32: the table the reference builds for complex64 input (the integer diagonal cast to float32,
    the double-precision square root rounded once, the boundary condition subtracted in float32)."""
    ctx = get_context(N)
    if np.dtype(dtype) == np.float32 and single_precision_on_device():
        lap32 = np.zeros((N, N, 2), dtype=np.float32)
        _lib.check(ctx._lib.qf_c64_laplacian_table(ctx.handle, int(bool(bc)), ptr(lap32)))
        return lap32
    lap = np.zeros((N, N, 2), dtype=np.float64)
    _lib.check(ctx._lib.qf_laplacian_table(ctx.handle, int(bool(bc)), ptr(lap)))
    return lap.astype(dtype, copy=False)


def solve_poisson(W, reduce=select_first):
    """Solve Delta P = W (quflow/laplacian/cpu.py:681-734).  The returned array is a
    persistent buffer that the caller may mutate and that the next call overwrites."""
    W = np.asarray(W)
    if W.ndim >= 3:
        W = reduce(W)
    in_dtype = W.dtype if W.dtype in (np.complex64, np.complex128) else np.complex128
    if in_dtype == np.complex64 and single_precision_on_device():
        # float32 tables, float32 Thomas solve, complex64 result (cpu.py:725-734)
        if W.ndim != 2 or W.shape[0] != W.shape[1]:
            raise ValueError("W must be a square matrix, got shape %s" % (W.shape,))
        W32 = np.ascontiguousarray(W, dtype=np.complex64)
        N = W32.shape[-1]
        ctx = get_context(N)
        P32 = _out_buffer(N, np.complex64)
        _lib.check(ctx._lib.qf_c64_solve_poisson(ctx.handle, ptr(W32), ptr(P32), int(_SKEW_HERM_)))
        return P32
    Wc = as_c128(W, "W")
    N = Wc.shape[-1]
    ctx = get_context(N)
    P = _out_buffer(N, np.complex128)
    _lib.check(ctx._lib.qf_solve_poisson(ctx.handle, ptr(Wc), ptr(P), int(_SKEW_HERM_)))
    if in_dtype == np.complex64:
        P32 = _out_buffer(N, np.complex64)
        P32[...] = P
        return P32
    return P


def laplace(P):
    """Apply the quantized Laplacian (quflow/laplacian/cpu.py:628-669, dense branch)."""
    if np.asarray(P).dtype == np.complex64 and single_precision_on_device():
        P32 = np.ascontiguousarray(P, dtype=np.complex64)
        if P32.ndim != 2 or P32.shape[0] != P32.shape[1]:
            raise ValueError("P must be a square matrix, got shape %s" % (P32.shape,))
        W32 = result_array(P32.shape, P32.dtype, "laplace")
        ctx = get_context(P32.shape[-1])
        _lib.check(ctx._lib.qf_c64_laplace(ctx.handle, ptr(P32), ptr(W32)))
        return W32
    Pc = as_c128(P, "P")
    N = Pc.shape[-1]
    ctx = get_context(N)
    W = result_array(Pc.shape, Pc.dtype, "laplace")      # (a new array per call unless the last one was dropped)
    _lib.check(ctx._lib.qf_laplace(ctx.handle, ptr(Pc), ptr(W)))
    return W.astype(np.asarray(P).dtype, copy=False) if np.asarray(P).dtype == np.complex64 else W


def _table_key(*parts):
    key = hash(parts) & 0xFFFFFFFFFFFFFFFF
    return key or 1


def _is_c64(W):
    return np.asarray(W).dtype == np.complex64 and single_precision_on_device()


def _solve_with_table(table, key, W):
    if _is_c64(W):
        # complex64 data: float32 table (built in float32 by the callers, as cpu.py:760,809 do with
        # dtype=type(W[0,0].real)) and the float32 solve
        W32 = np.ascontiguousarray(W, dtype=np.complex64)
        if W32.ndim != 2 or W32.shape[0] != W32.shape[1]:
            raise ValueError("W must be a square matrix, got shape %s" % (W32.shape,))
        ctx = get_context(W32.shape[-1])
        tab32 = np.ascontiguousarray(table, dtype=np.float32)
        P32 = np.zeros_like(W32)
        _lib.check(ctx._lib.qf_c64_solve_tridiagonal(ctx.handle, ptr(tab32), ptr(W32), ptr(P32), int(_SKEW_HERM_)))
        return P32
    Wc = as_c128(W, "W")
    N = Wc.shape[-1]
    ctx = get_context(N)
    table = np.ascontiguousarray(table, dtype=np.float64)
    P = np.zeros_like(Wc)
    _lib.check(ctx._lib.qf_solve_tridiagonal(ctx.handle, ptr(table), ctypes.c_ulonglong(key), ptr(Wc), ptr(P),
                                             int(_SKEW_HERM_)))
    return P


class _LRU(collections.OrderedDict):
    """Host tables are 16 N^2 bytes each (16 MiB at N=1024): keep the few a run alternates between
    (two half steps of a Strang splitting, a couple of sizes), not one per step size ever seen."""

    def __init__(self, maxlen=8):
        super().__init__()
        self.maxlen = maxlen

    def lookup(self, key, build):
        if key in self:
            self.move_to_end(key)
            return self[key]
        val = build()
        self[key] = val
        while len(self) > self.maxlen:
            self.popitem(last=False)
        return val


_table_cache = _LRU()
_plain_table_cache = _LRU(4)


def _shifted_table(N, c0, c1, dtype=np.float64):
    """c0*I - c1*Delta as an (N,N,2) table: the heat/helmholtz/viscdamp operators (cpu.py:765-769), in the
    arithmetic of `dtype` (float32 for complex64 data: the reference's `lap.copy()` is a float32 array then)."""
    dtype = np.dtype(dtype)
    def build():
        lap = _plain_table_cache.lookup((N, dtype.str), lambda: laplacian(N, bc=False, dtype=dtype))
        tab = lap.copy()
        tab[:, :, 0] = c0
        tab[:, :, 1] = 0.0
        tab -= c1 * lap
        return tab
    return _table_cache.lookup((N, float(c0), float(c1), dtype.str), build)


def _real_dtype(W):
    return np.float32 if _is_c64(W) else np.float64


def solve_helmholtz(W, alpha=1.0):
    """(1 - alpha Delta) P = W, quflow/laplacian/cpu.py:784-826."""
    N = np.asarray(W).shape[-1]
    return _solve_with_table(_shifted_table(N, 1.0, alpha, _real_dtype(W)), _table_key("helm", N, float(alpha)), W)


def solve_heat(h_times_nu, W0):
    """(1 - h nu Delta) W = W0, quflow/laplacian/cpu.py:737-781."""
    N = np.asarray(W0).shape[-1]
    return _solve_with_table(_shifted_table(N, 1.0, h_times_nu, _real_dtype(W0)), _table_key("helm", N, float(h_times_nu)), W0)


_globalqg_cache = _LRU(4)


def _globalqg_table(N, gamma, dtype=np.float64):
    """The (N,N,2) table of Delta + gamma Z . Z: the Laplacian table with (gamma/2)(z_i^2 + z_j^2) taken off its diagonal
    coefficient, z = hbar*(-s..s) the diagonal of the third Cartesian generator (cpu.py:829-877)."""
    dtype = np.dtype(dtype)
    def build():
        s = (N - 1) / 2
        zvec = _geometry.hbar(N) * np.arange(-s, s + 1)
        tab = laplacian(N, bc=False, dtype=dtype).copy()
        tab[:, :, 0] -= (gamma / 2.0) * zvec ** 2
        tab[:, :, 0] -= (gamma / 2.0) * zvec[:, np.newaxis] ** 2
        return tab
    return _globalqg_cache.lookup((N, float(gamma), dtype.str), build)


def solve_globalqg(W, gamma=1.0):
    """Delta P + gamma Z P Z = W, quflow/laplacian/cpu.py:829-877 (the table of `_globalqg_table`); same device Thomas
    kernel."""
    N = np.asarray(W).shape[-1]
    return _solve_with_table(_globalqg_table(N, gamma, _real_dtype(W)), _table_key("gqg", N, float(gamma)), W)


def solve_viscdamp(h, W0, nu=1e-4, alpha=0.01, force=None, theta=1):
    """Theta scheme for W' - nu Delta W + alpha W = F, quflow/laplacian/cpu.py:880-943."""
    W0 = np.asarray(W0)
    N = W0.shape[-1]
    tab = _shifted_table(N, 1.0 + h * alpha * theta, h * nu * theta, _real_dtype(W0))
    if theta == 1:
        Wrhs = W0.copy()
    else:
        Wrhs = (1.0 - alpha * h * (1 - theta)) * W0
        Wrhs += (nu * h * (1 - theta)) * laplace(W0)
    if force is not None:
        Wrhs += h * force
    return _solve_with_table(tab, _table_key("visc", N, float(h), float(nu), float(alpha), float(theta)), Wrhs)


class ViscDampStep:
    """`strang_splitting=ViscDampStep(nu, alpha)`: the viscous / damped half step
    `lambda h, W: solve_viscdamp(h, W, nu, alpha)` of the reference's forced-turbulence runs
    (cpu.py:880-943, theta = 1, no force) as an object the device stepper recognises: between device
    steps it is applied to the resident state (no PCIe).  Called directly it is that lambda."""

    def __init__(self, nu=1e-4, alpha=0.01):
        self.nu = float(nu)
        self.alpha = float(alpha)

    def __call__(self, h, W):
        return solve_viscdamp(h, W, nu=self.nu, alpha=self.alpha)

    def table_and_key(self, N, h):
        """The (N,N,2) table of 1 + h alpha - h nu Delta and its cache key."""
        return (_shifted_table(N, 1.0 + h * self.alpha, h * self.nu),
                _table_key("visc", N, float(h), self.nu, self.alpha, 1.0))

    def apply_resident(self, ctx, h):
        """W <- (1 + h alpha - h nu Delta)^-1 W on the context's state."""
        tab, key = self.table_and_key(ctx.N, h)
        _lib.check(ctx._lib.qf_solve_tridiagonal(ctx.handle, ptr(np.ascontiguousarray(tab)), ctypes.c_ulonglong(key),
                                                 None, None, int(_SKEW_HERM_)))


class PoissonHIP:
    """Device Poisson operator with the constructor/call shape of the reference's
    DiagTriDiagOp (quflow/experimental/cuda.py:166-189, quflow/simulation.py:554-562):
    `PoissonHIP(N, dtype)(P_out, W_in)`; also usable as `hamiltonian(W) -> P`."""

    __name__ = "quhip"

    def __init__(self, N, dtype=np.complex128, device=None):
        self.N = int(N)
        self.dtype = np.dtype(dtype)
        self.ctx = get_context(self.N, device)

    def __call__(self, *args):
        if len(args) == 1:
            return solve_poisson(args[0])
        P_out, W_in = args
        P_out[...] = solve_poisson(W_in)
        return None

    solve_poisson = staticmethod(solve_poisson)
    laplace = staticmethod(laplace)
    select_skewherm = staticmethod(select_skewherm)


def coriolis(N, omega):
    """The offset matrix of solid-body rotation with angular velocity `omega`: shr2mat of the function 2 omega cos(theta),
    i.e. of the one real coefficient 2 omega / sqrt(3) at elm2ind(1, 0) -- the convention shr2fun inverts: a unit
    coefficient there is the function sqrt(3) cos(theta) (the transforms carry the factor sqrt(4 pi) of Y_10 =
    sqrt(3 / (4 pi)) cos(theta)).  Dense, diagonal, skew-Hermitian and trace-free; it is 2 omega X3, twice omega times the
    matrix of the Cartesian coordinate function x3 = cos(theta) (cartesian_generators).  The basis element T_10 =
    elmr2mat(1, 0, N) is written in its closed form i sqrt(12 / (N^2 - 1)) diag(k - (N-1)/2) (unit norm_L2, last entry
    positive: the reference's orientation rule), so that no quantization basis -- N^3/3 doubles -- is needed for one
    diagonal."""
    N = int(N)
    d = (np.arange(N, dtype=np.float64) - (N - 1) / 2) * np.sqrt(12.0 / (N * N - 1.0))
    F = np.zeros((N, N), dtype=np.complex128)
    F[np.arange(N), np.arange(N)] = (2.0 * float(omega) / np.sqrt(3.0)) * 1j * d
    return F


def _content_key(tag, a):
    """A 64-bit id of a host array for the library's caches, from its WHOLE content: the tag, the dtype, the shape and every
    byte (SHA-256, first 8 bytes; never 0, which the library reads as "always upload").  The library reuses what a context
    holds when the key repeats, and its own fingerprint reads 4096 strided entries only: the key is what tells two contents
    apart, so it must not sample.  One pass over the array: computed once, by the constructors, never per install."""
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(("%s|%s|%r|" % (tag, a.dtype.str, a.shape)).encode())
    h.update(a.reshape(-1).view(np.uint8))
    return int.from_bytes(h.digest()[:8], "little") or 1


def _owned(a, dtype):
    """A C-contiguous copy of `a` that nobody else holds, write-protected: what an immutable instance keeps and keys."""
    a = np.array(a, dtype=dtype, order="C")
    a.setflags(write=False)
    return a


class TridiagonalHamiltonian:
    """`hamiltonian=` of the steppers for P = T^-1 (W - F): T a tridiagonal operator given by its (N,N,2) coefficient
    table (the layout of `laplacian(N)`: diagonal and coupling coefficient per entry), F an optional fixed offset matrix
    (Coriolis term `coriolis(N, omega)`, topography, ...).  The flow on a rotating sphere, the global quasi-geostrophic
    model and Charney-Hasegawa-Mima are instances:

        H = TridiagonalHamiltonian.poisson(N, offset=coriolis(N, omega))          # Delta P = W - F
        H = TridiagonalHamiltonian.globalqg(N, gamma, offset=...)                 # Delta P + gamma Z P Z = W - F
        H = TridiagonalHamiltonian.shifted(N, -alpha, -1.0)                       # (Delta - alpha) P = W

    isomp / isomp_fixedpoint, euler / heun / rk4, isomp_simple / isomp_quasinewton, DeviceTrajectory, DeviceEnsemble and
    quflow_amd.solve recognise an instance and install it on the device context they run on (qf_set_hamiltonian): the
    table is factorised once, the offset stays in HBM and is subtracted inside the solve kernel, and the trajectory never
    visits the host.  That holds for complex128 data with the skew-Hermitian flags on; elsewhere (complex64, the general
    commutator, magmp) an instance is the callable `H(W) -> P` it also is and takes the foreign-Hamiltonian route.

    The offset must be EXACTLY skew-Hermitian (the skew-Hermitian solve reads the upper triangle of its right-hand side
    only): ValueError otherwise.

    Instances are immutable: `table` and `offset` are write-protected copies of what was passed, and `table_key` /
    `offset_key`, by which a context recognises what it already holds, are digests of their whole content, computed here
    once.  A run that edits its topography makes a new instance."""

    def __init__(self, table, offset=None):
        table = _owned(table, np.float64)
        if table.ndim != 3 or table.shape[0] != table.shape[1] or table.shape[2] != 2 or table.shape[0] < 2:
            raise ValueError("table must be an (N,N,2) coefficient table, got shape %s" % (table.shape,))
        self.N = int(table.shape[0])
        self.table = table
        self.builtin = False         # the table is the built-in Laplacian's: the context's own factors serve
        self.offset = None
        if offset is not None:
            offset = _owned(offset, np.complex128)
            if offset.shape != (self.N, self.N):
                raise ValueError("offset must be (%d, %d), got %s" % (self.N, self.N, offset.shape))
            if not np.array_equal(offset, -offset.conj().T):
                raise ValueError("offset must be exactly skew-Hermitian (F == -F^H entry by entry): project it with "
                                 "F = (F - F^H) / 2 first")
            self.offset = offset
        # (the instance owns write-protected copies: the keys, computed here once from the whole content, stay true)
        self.table_key = _content_key("ham_table", self.table)
        self.offset_key = 0 if self.offset is None else _content_key("ham_offset", self.offset)

    def __setstate__(self, state):
        self.__dict__.update(state)
        for a in (self.table, self.offset):       # (numpy unpickles arrays writeable)
            if a is not None:
                a.setflags(write=False)
        # (keyed again, not trusted: a simulation stored by an earlier version carries keys of sampled entries)
        self.table_key = _content_key("ham_table", self.table)
        self.offset_key = 0 if self.offset is None else _content_key("ham_offset", self.offset)

    @classmethod
    def poisson(cls, N, offset=None):
        """Delta P = W - F with the Laplacian of solve_poisson (bc=True): the built-in factors, plus an offset."""
        self = cls(laplacian(int(N), bc=True), offset)
        self.builtin = True
        return self

    @classmethod
    def globalqg(cls, N, gamma, offset=None):
        """Delta P + gamma Z P Z = W - F: the operator of solve_globalqg (cpu.py:829-877)."""
        return cls(_globalqg_table(int(N), gamma), offset)

    @classmethod
    def shifted(cls, N, c0, c1, offset=None):
        """(c0 I - c1 Delta) P = W - F, the table of solve_helmholtz / solve_heat / solve_viscdamp; Charney-Hasegawa-Mima
        (Delta - alpha) P = W is c0 = -alpha, c1 = -1."""
        return cls(_shifted_table(int(N), c0, c1), offset)

    # ---- installing on a device context (the steppers and the device objects call these)
    def check_size(self, N):
        if int(N) != self.N:
            raise ValueError("the Hamiltonian was built for N=%d, the state has N=%d" % (self.N, int(N)))

    def install(self, ctx):
        self.check_size(ctx.N)
        _lib.check(ctx._lib.qf_set_hamiltonian(ctx.handle, None if self.builtin else ptr(self.table),
                                               ctypes.c_ulonglong(self.table_key),
                                               None if self.offset is None else ptr(self.offset),
                                               ctypes.c_ulonglong(self.offset_key)))

    @staticmethod
    def uninstall(ctx):
        if ctx.handle:
            _lib.check(ctx._lib.qf_clear_hamiltonian(ctx.handle))

    # ---- the reference's `hamiltonian(W) -> P` protocol
    def __call__(self, W):
        W = np.asarray(W)
        if W.ndim >= 3:
            W = select_first(W)
        if W.ndim != 2 or W.shape[0] != W.shape[1]:
            raise ValueError("W must be a square matrix, got shape %s" % (W.shape,))
        self.check_size(W.shape[-1])
        if not _SKEW_HERM_ or _is_c64(W):
            # the general solve / complex64 data: the host-in, host-out table solve of W - F
            rhs = W if self.offset is None else W - self.offset.astype(W.dtype, copy=False)
            tab = self.table.astype(np.float32) if _is_c64(W) else self.table
            return _solve_with_table(tab, self.table_key, rhs)
        Wc = as_c128(W, "W")
        ctx = get_context(self.N)
        P = np.empty_like(Wc)
        self.install(ctx)
        try:
            _lib.check(ctx._lib.qf_hamiltonian(ctx.handle, ptr(Wc), ptr(P)))
        finally:
            self.uninstall(ctx)
        return P.astype(W.dtype, copy=False) if W.dtype == np.complex64 else P


def installable(h):
    """`h` is a TridiagonalHamiltonian and the process is in the mode in which the device follows an installed one: the
    skew-Hermitian solve (select_skewherm(True), the default)."""
    return isinstance(h, TridiagonalHamiltonian) and _SKEW_HERM_


class AffineForcing:
    """`forcing=` of the steppers for the forcing that is affine in the state,

        F(P, W) = F0 + a_W W + a_P P + a_lap Delta W          (a_* real, F0 a fixed skew-Hermitian pattern)

    -- a fixed pattern, Rayleigh friction (a_W < 0), a large-scale drag on the stream function (a_P) and viscosity
    (a_lap > 0) -- as an object the device follows: isomp / isomp_fixedpoint and euler / heun / rk4 on an (N,N) complex128
    state in skew-Hermitian mode, DeviceTrajectory and quflow_amd.solve install it on the device context they run on
    (qf_set_forcing), where one kernel forms the force term from the matrices the loop already holds; nothing crosses
    PCIe for it.  Elsewhere -- stacks, magmp, select_skewherm(False), complex64 data -- an instance is the callable
    `forcing(P, W)` it also is and takes the host-hook route of any callable.

    The order of operations is fixed.  Where a loop evaluates the forcing at a matrix X (Whalf in the isomp loop, the stage
    argument in euler / heun / rk4) with the stream matrix Ph as the loop holds it, a stream-matrix scale pscale and an
    output scale s, the device computes per entry, on real and imaginary parts separately, every product and sum rounded on
    its own (no fused multiply-add):

        p = Ph * pscale
        f = F0[e]                        (0 when there is no F0)
        f = f + a_W * X[e]               (term skipped entirely when a_W == 0.0)
        f = f + a_P * p                  (skipped when a_P == 0.0)
        f = f + a_lap * (Delta X)[e]     (skipped when a_lap == 0.0; Delta X as quflow_amd.laplace gives it)
        out = s * f

    isomp loop: pscale = 1 / (dt / (2 hbar)), s = dt / 2 (what the host-hook route does to P before and to F behind the
    call: isospectral.py:512-520); explicit loops and `__call__`: pscale = s = 1.  A numpy callable that repeats these lines
    on `.real` / `.imag` float64 arrays, with Delta X from quflow_amd.laplace, gives the same numbers bit for bit.

    F0 must be finite and EXACTLY skew-Hermitian (F0 == -F0^H entry by entry), the coefficients finite real numbers:
    ValueError / TypeError otherwise.  Instances are immutable; a run that redraws its pattern makes a new one per chunk
    (DeviceTrajectory.set_forcing)."""

    def __init__(self, F0=None, a_W=0.0, a_P=0.0, a_lap=0.0):
        coeff = []
        for name, a in (("a_W", a_W), ("a_P", a_P), ("a_lap", a_lap)):
            if isinstance(a, (complex, np.complexfloating)) or isinstance(a, (str, bytes, bool)) or not np.isscalar(a):
                raise TypeError("%s must be a real number, got %r" % (name, a))
            a = float(a)
            if not np.isfinite(a):
                raise ValueError("%s must be finite, got %r" % (name, a))
            coeff.append(a)
        self.a_W, self.a_P, self.a_lap = coeff
        self.F0 = None
        self.N = None
        self.F0_key = 0
        if F0 is not None:
            F0 = np.array(F0, dtype=np.complex128, order="C")
            if F0.ndim != 2 or F0.shape[0] != F0.shape[1] or F0.shape[0] < 2:
                raise ValueError("F0 must be an (N,N) matrix, got shape %s" % (F0.shape,))
            if not np.all(np.isfinite(F0.view(np.float64))):
                raise ValueError("F0 must be finite")
            if not np.array_equal(F0, -F0.conj().T):
                raise ValueError("F0 must be exactly skew-Hermitian (F0 == -F0^H entry by entry): project it with "
                                 "F0 = (F0 - F0^H) / 2 first")
            F0.setflags(write=False)
            self.F0 = F0
            self.N = int(F0.shape[0])
            self.F0_key = _content_key("forcing_f0", F0)

    def __setstate__(self, state):
        self.__dict__.update(state)
        if self.F0 is not None:                   # (numpy unpickles arrays writeable)
            self.F0.setflags(write=False)
            # (keyed again, not trusted: a simulation stored by an earlier version carries a key of sampled entries)
            self.F0_key = _content_key("forcing_f0", self.F0)

    def check_size(self, N):
        if self.N is not None and int(N) != self.N:
            raise ValueError("the forcing was built for N=%d, the state has N=%d" % (self.N, int(N)))

    # ---- installing on a device context (the steppers and the device objects call these)
    def install(self, ctx):
        self.check_size(ctx.N)
        _lib.check(ctx._lib.qf_set_forcing(ctx.handle, None if self.F0 is None else ptr(self.F0),
                                           ctypes.c_ulonglong(self.F0_key), self.a_W, self.a_P, self.a_lap))

    @staticmethod
    def uninstall(ctx):
        if ctx.handle:
            _lib.check(ctx._lib.qf_clear_forcing(ctx.handle))

    # ---- the reference's `forcing(P, W) -> F` protocol, through the same kernel (pscale = s = 1)
    def __call__(self, P, W):
        W = np.asarray(W)
        P = np.asarray(P)
        if W.ndim == 3:
            if P.ndim == 3 and P.shape[0] != W.shape[0]:
                raise ValueError("P %s does not go with the stack W %s" % (P.shape, W.shape))
            return np.stack([self(P[j] if P.ndim == 3 else P, W[j]) for j in range(W.shape[0])])
        Wc = as_c128(W, "W")
        Pc = as_c128(P, "P")
        if Pc.shape != Wc.shape:
            raise ValueError("operands could not be broadcast together with shapes %s %s" % (Pc.shape, Wc.shape))
        self.check_size(Wc.shape[-1])
        ctx = get_context(Wc.shape[-1])
        F = np.empty_like(Wc)
        self.install(ctx)
        try:
            _lib.check(ctx._lib.qf_forcing(ctx.handle, ptr(Pc), ptr(Wc), ptr(F)))
        finally:
            self.uninstall(ctx)
        return F


_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 on uint64 arrays holding 32-bit words: `counter` four words (each a scalar or an array, broadcast
    together), `key` two.  Returns the four output words as uint64 arrays.  The host mirror of the device generator of
    StochasticForcing (csrc/stochastic.hip)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _MASK32 for c in counter])
    k0, k1 = (np.uint64(int(k) & 0xFFFFFFFF) for k in key)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2            # (32 x 32 bits: exact in uint64)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> s32) ^ c3 ^ k1, p0 & _MASK32
        k0 = (k0 + _PHILOX_W0) & _MASK32
        k1 = (k1 + _PHILOX_W1) & _MASK32
    return c0, c1, c2, c3


def philox_uniforms(x0, x1, x2, x3):
    """u in (0, 1] and v in [0, 1) from the four output words, every operation exact in double:
    u = ((x0 >> 5) 2^26 + (x1 >> 6) + 1) 2^-53,  v = ((x2 >> 5) 2^26 + (x3 >> 6)) 2^-53."""
    x0, x1, x2, x3 = (np.asarray(x, dtype=np.uint64) for x in (x0, x1, x2, x3))
    u = ((x0 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (x1 >> np.uint64(6)).astype(np.float64) + 1.0) * 2.0 ** -53
    v = ((x2 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (x3 >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    return u, v


_STOCHASTIC_ROUTES = ("a StochasticForcing is followed by isomp / isomp_fixedpoint on an (N,N) complex128 host array in "
                      "skew-Hermitian mode (select_skewherm(True)), by DeviceTrajectory(forcing=...) / .set_forcing(...) and by "
                      "solve on such a run; elsewhere pass forcing=sf.as_callable(dt, N) to a stepper that takes a host callable")


def _uint64_arg(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise TypeError("%s must be an integer, got %r" % (name, v))
    v = int(v)
    if not 0 <= v < 2 ** 64:
        raise ValueError("%s must lie in [0, 2^64), got %d" % (name, v))
    return v


class StochasticForcing:
    """`forcing=` for stochastic band-limited forcing, white in time, drawn and applied on the device:

        F(P, W) = F0_n + a_W W + a_P P + a_lap Delta W

    where over the step n -> n + 1 of size dt the pattern is F0_n = shr2mat(omega_n, N) with

        omega_n[l^2 + l + m] = (sigma_l * (1 / sqrt(dt))) * xi_n(l, m)     l_min <= l <= l_max, -l <= m <= l; zero elsewhere,

    xi iid N(0,1).  The generator is counter based (Philox4x32-10, key = seed, counter = (n, (l^2 + l + m) >> 1); Box-Muller:
    cosine for even l^2 + l + m, sine for odd; include/quflow_hip.h has every constant), so a coefficient depends on
    (seed, n, l, m) alone -- not on N, the band, how the run is cut into calls -- and `draw_host` repeats it in numpy.  The
    affine terms are AffineForcing's, in its order of operations; F0_n is constant over a step's fixed-point iterations.

    `sigma`: one amplitude for the band or one per l (l_min .. l_max), finite and >= 0.  `seed`, `step`: integers in
    [0, 2^64).  `.step` is the counter n of the next step a run takes: every call that ran with the forcing installed leaves
    it advanced by its steps, and the object pickles with it -- a resumed run carries on the same noise sequence.

    FOLLOWED by isomp / isomp_fixedpoint on an (N,N) complex128 host array in skew-Hermitian mode,
    DeviceTrajectory(forcing=...) / .set_forcing(...), and solve on such runs (resident by default).  Everywhere else --
    stacks, magmp, complex64, select_skewherm(False), euler / heun / rk4, isomp_simple / isomp_quasinewton, DeviceEnsemble --
    it raises NotImplementedError; `as_callable(dt, N)` is the host callable with the same numbers for those routes."""

    def __init__(self, l_min, l_max, sigma, seed, a_W=0.0, a_P=0.0, a_lap=0.0, step=0):
        for name, v in (("l_min", l_min), ("l_max", l_max)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError("%s must be an integer, got %r" % (name, v))
        l_min, l_max = int(l_min), int(l_max)
        if not 1 <= l_min <= l_max:
            raise ValueError("the band must satisfy 1 <= l_min <= l_max (l = 0 is the trace), got l_min=%d, l_max=%d"
                             % (l_min, l_max))
        if l_max > 8191:
            raise ValueError("l_max must be at most 8191 (N <= 8192), got %d" % l_max)
        if sigma is None or isinstance(sigma, (str, bytes, bool)) or np.iscomplexobj(sigma):
            raise TypeError("sigma must be a real number or one real number per l of the band, got %r" % (sigma,))
        try:
            sig = np.array(sigma, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError("sigma must be a real number or one real number per l of the band, got %r" % (sigma,))
        nl = l_max - l_min + 1
        if sig.ndim == 0:
            sig = np.full(nl, float(sig))
        if sig.shape != (nl,):
            raise ValueError("sigma must be a scalar or have one value per l of the band (%d), got shape %s" % (nl, sig.shape))
        if not np.all(np.isfinite(sig)) or np.any(sig < 0):
            raise ValueError("sigma must be finite and >= 0")
        coeff = []
        for name, a in (("a_W", a_W), ("a_P", a_P), ("a_lap", a_lap)):
            if isinstance(a, (complex, np.complexfloating)) or isinstance(a, (str, bytes, bool)) or not np.isscalar(a):
                raise TypeError("%s must be a real number, got %r" % (name, a))
            a = float(a)
            if not np.isfinite(a):
                raise ValueError("%s must be finite, got %r" % (name, a))
            coeff.append(a)
        self.l_min, self.l_max = l_min, l_max
        self.sigma = np.ascontiguousarray(sig)
        self.sigma.setflags(write=False)
        self.seed = _uint64_arg("seed", seed)
        self.step = _uint64_arg("step", step)
        self.a_W, self.a_P, self.a_lap = coeff

    def check_size(self, N):
        if self.l_max > int(N) - 1:
            raise ValueError("the band reaches l_max=%d, a state of size N=%d carries l <= %d" % (self.l_max, int(N), int(N) - 1))

    # ---- installing on a device context (the steppers and the device objects call these)
    def install(self, ctx):
        from .quantization import slab_bytes
        self.check_size(ctx.N)
        sig = np.array(self.sigma)
        _lib.check(ctx._lib.qf_set_stochastic_forcing(ctx.handle, self.l_min, self.l_max, ptr(sig), ctypes.c_ulonglong(self.seed),
                                                      ctypes.c_ulonglong(self.step), self.a_W, self.a_P, self.a_lap,
                                                      ctypes.c_longlong(slab_bytes())))

    def sync(self, ctx):
        """Read the counter back from the context this forcing is installed on (qf_stochastic_tell)."""
        n = ctypes.c_ulonglong()
        _lib.check(ctx._lib.qf_stochastic_tell(ctx.handle, ctypes.byref(n)))
        self.step = int(n.value)
        return self.step

    @staticmethod
    def uninstall(ctx):
        if ctx.handle:
            _lib.check(ctx._lib.qf_clear_forcing(ctx.handle))

    def __call__(self, *args, **kwargs):
        raise NotImplementedError("a StochasticForcing is no host callable forcing(P, W): " + _STOCHASTIC_ROUTES)

    # ---- what the device draws, downloaded (qf_stochastic_pattern); the run's counter is not touched
    def _device_pattern(self, n, dt, N, want_pattern):
        n = _uint64_arg("n", n)
        N = int(N)
        self.check_size(N)
        ctx = get_context(N)
        omega = np.zeros((self.l_max + 1) ** 2, dtype=np.float64)
        F0 = np.zeros((N, N), dtype=np.complex128) if want_pattern else None
        self.install(ctx)
        try:
            _lib.check(ctx._lib.qf_stochastic_pattern(ctx.handle, ctypes.c_ulonglong(n), float(dt), ptr(omega),
                                                      None if F0 is None else ptr(F0)))
        finally:
            self.uninstall(ctx)
        return omega, F0

    def coefficients(self, n, dt, N):
        """omega_n for step size dt as the device draws it: (l_max + 1)^2 real coefficients, index l^2 + l + m."""
        return self._device_pattern(n, dt, N, False)[0]

    def pattern(self, n, dt, N):
        """F0_n = shr2mat(omega_n, N) as the device forms it for the run: an (N,N) complex128 skew-Hermitian matrix."""
        return self._device_pattern(n, dt, N, True)[1]

    def draw_host(self, n, dt):
        """The numpy mirror of the device draw: omega_n, (l_max + 1)^2 doubles.  Philox on uint64 arrays, then the formulas
        of the class docstring, operation by operation; differs from `coefficients` only by the device's log / sincos
        against numpy's."""
        n = _uint64_arg("n", n)
        dt = float(dt)
        if not dt > 0.0 or not np.isfinite(dt):
            raise ValueError("dt must be positive and finite, got %r" % dt)
        q = np.arange(self.l_min ** 2, (self.l_max + 1) ** 2, dtype=np.int64)
        x = philox4x32_10((n & 0xFFFFFFFF, n >> 32, (q >> 1).astype(np.uint64), 0), (self.seed & 0xFFFFFFFF, self.seed >> 32))
        u, v = philox_uniforms(*x)
        r = np.sqrt(-2.0 * np.log(u))
        t = 6.283185307179586 * v
        xi = np.where(q % 2 == 0, r * np.cos(t), r * np.sin(t))
        el = np.floor(np.sqrt(q.astype(np.float64))).astype(np.int64)      # (q < 2^26: the double root floors exactly)
        inv = 1.0 / np.sqrt(dt)
        s = self.sigma[el - self.l_min] * inv
        omega = np.zeros((self.l_max + 1) ** 2, dtype=np.float64)
        omega[q] = s * xi
        return omega

    def as_callable(self, dt, N, time0=0.0):
        """The time-dependent host callable f(P, W, time) with this forcing's numbers, for the routes the device does not
        follow (pass `time=` to the stepper).  A stepper evaluates the forcing of the step that starts at time t at
        t + dt/2, so the step index is n = step + round((time - time0 - dt/2) / dt), clamped at 0, with `step` the counter at
        the time of this call and time0 the time of that step's start; the pattern is pattern(n, dt, N), then the affine
        lines in AffineForcing's order.  A pure function of its arguments: a stepper's probing call consumes nothing."""
        dt, N, time0, step0 = float(dt), int(N), float(time0), self.step
        self.check_size(N)
        a_W, a_P, a_lap = self.a_W, self.a_P, self.a_lap
        last = {}

        def forcing(P, W, time):
            W = np.asarray(W)
            if W.ndim == 3:
                P = np.asarray(P)
                return np.stack([forcing(P[j] if P.ndim == 3 else P, W[j], time) for j in range(W.shape[0])])
            n = max(step0 + int(round((float(time) - time0 - dt / 2) / dt)), 0)
            if last.get("n") != n:
                last["F0"] = self.pattern(n, dt, N)
                last["n"] = n
            F0 = last["F0"]
            fr, fi = F0.real.copy(), F0.imag.copy()
            if a_W != 0.0:
                fr = fr + a_W * W.real
                fi = fi + a_W * W.imag
            if a_P != 0.0:
                fr = fr + a_P * P.real
                fi = fi + a_P * P.imag
            if a_lap != 0.0:
                L = laplace(np.ascontiguousarray(W, dtype=np.complex128))
                fr = fr + a_lap * L.real
                fi = fi + a_lap * L.imag
            out = np.empty(W.shape, dtype=np.complex128)
            out.real = fr
            out.imag = fi
            return out
        return forcing

    # ---- expected injection rates.  The basis elements T_lm (elmr2mat) have unit norm_L2 and Delta T_lm = -l(l+1) T_lm, so
    # over one step dt F0_n = sqrt(dt) sum sigma_l xi T_lm adds on average dt/2 sum_l (2l+1) sigma_l^2 of enstrophy
    # <W, W>/2 and dt/2 sum_l (2l+1) sigma_l^2 / (l(l+1)) of energy -<W, Delta^-1 W>/2 (the cross terms vanish in the mean)
    def energy_rate(self):
        """Expected energy injection per unit time: 1/2 sum_l (2l + 1) sigma_l^2 / (l (l + 1))."""
        el = np.arange(self.l_min, self.l_max + 1, dtype=np.float64)
        return float(0.5 * np.sum((2 * el + 1) * self.sigma ** 2 / (el * (el + 1))))

    def enstrophy_rate(self):
        """Expected enstrophy injection per unit time: 1/2 sum_l (2l + 1) sigma_l^2."""
        el = np.arange(self.l_min, self.l_max + 1, dtype=np.float64)
        return float(0.5 * np.sum((2 * el + 1) * self.sigma ** 2))


DEVICE_FORCINGS = (AffineForcing, StochasticForcing)      # what a device context follows once installed


def forcing_installable(f):
    """`f` is an AffineForcing or a StochasticForcing and the process is in the mode in which the device follows an installed
    one: the skew-Hermitian solve (select_skewherm(True), the default)."""
    return isinstance(f, DEVICE_FORCINGS) and _SKEW_HERM_
