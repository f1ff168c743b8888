"""The streamed quantization basis (qf_basis_stream, quantization.hip: k_basis_slab and the slab forms of k_block_matvec /
k_block_vecmat): no resident basis, the blocks a transform needs rebuilt slab by slab.

  * N <= 1025: on ONE context holding the resident basis, every transform and its NULL forms give the same bits with the
    mode off and on, at every band limit of the large tests and at three slab budgets (one block per slab, a few, all in
    one).  The column arithmetic is the resident kernel's and the reductions run in the same order, so nothing but
    equality is accepted.
  * N = 4096 and 8192, where no resident basis fits: read-out columns against the tridiagonal blocks and LAPACK, the
    transforms on sampled blocks against the extended-precision helpers, round trips, and trajectories that start from
    and write out coefficients.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.linalg import eigh_tridiagonal

from oracle import quantization_oracle as qo
from test_hip_quantization_large import (ELMAX, EPS, SQRT2, _idx, _n_omegas, _sampled_ms, _sgn, assert_within,
                                         band_limit, ref_mat2shr, ref_shr2mat)

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    if quflow_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return quflow_amd


class Raw:
    """The C entry points on one context (host arrays in and out; the NULL forms through the context's state)."""

    def __init__(self, ctx):
        from quflow_amd import _lib
        from quflow_amd.context import ptr
        self.ctx, self.N, self.lib, self.check, self.ptr = ctx, ctx.N, ctx._lib, _lib.check, ptr

    def mode(self, slab_bytes):
        self.check(self.lib.qf_basis_stream(self.ctx.handle, ctypes.c_longlong(int(slab_bytes))))

    def shr2mat(self, om):
        om = np.ascontiguousarray(om, dtype=np.float64)
        W = np.zeros((self.N, self.N), dtype=np.complex128)
        self.check(self.lib.qf_shr2mat(self.ctx.handle, self.ptr(om), ctypes.c_longlong(om.shape[0]), self.ptr(W)))
        return W

    def mat2shr(self, W, n):
        Wc = np.ascontiguousarray(W, dtype=np.complex128)
        om = np.zeros(n)
        self.check(self.lib.qf_mat2shr(self.ctx.handle, self.ptr(Wc), self.ptr(om), ctypes.c_longlong(n)))
        return om

    def shc2mat(self, om):
        om = np.ascontiguousarray(om, dtype=np.complex128)
        W = np.zeros((self.N, self.N), dtype=np.complex128)
        self.check(self.lib.qf_shc2mat(self.ctx.handle, self.ptr(om), self.ptr(W)))
        return W

    def mat2shc(self, W):
        Wc = np.ascontiguousarray(W, dtype=np.complex128)
        om = np.zeros(self.N * self.N, dtype=np.complex128)
        self.check(self.lib.qf_mat2shc(self.ctx.handle, self.ptr(Wc), self.ptr(om)))
        return om

    def upload(self, W):
        self.check(self.lib.qf_upload_W(self.ctx.handle, self.ptr(np.ascontiguousarray(W, dtype=np.complex128))))

    def download(self):
        W = np.zeros((self.N, self.N), dtype=np.complex128)
        self.check(self.lib.qf_download_W(self.ctx.handle, self.ptr(W)))
        return W

    def null_forms(self, om, W, n, L):
        """shr2mat(om) into the state; mat2shr(state) to the host; mat2shr(W) kept on the device -> shr2fun(NULL) and
        -> shr2mat(NULL) to the host."""
        om = np.ascontiguousarray(om, dtype=np.float64)
        self.check(self.lib.qf_shr2mat(self.ctx.handle, self.ptr(om), ctypes.c_longlong(om.shape[0]), None))
        state = self.download()
        self.upload(W)
        from_state = np.zeros(n)
        self.check(self.lib.qf_mat2shr(self.ctx.handle, None, self.ptr(from_state), ctypes.c_longlong(n)))
        Wc = np.ascontiguousarray(W, dtype=np.complex128)
        self.check(self.lib.qf_mat2shr(self.ctx.handle, self.ptr(Wc), None, ctypes.c_longlong(n)))
        f = np.zeros((L, 2 * L - 1))
        self.check(self.lib.qf_shr2fun(self.ctx.handle, None, ctypes.c_longlong(n), L, 1, self.ptr(f)))
        back = np.zeros((self.N, self.N), dtype=np.complex128)
        self.check(self.lib.qf_shr2mat(self.ctx.handle, None, ctypes.c_longlong(n), self.ptr(back)))
        return state, from_state, f, back


def _budgets(N, Nmax):
    """One block per slab (the budget is block 0 itself), a few blocks, everything in one slab."""
    b0 = 8 * N * Nmax
    return {"one": b0, "few": 3 * b0 + 8, "all": 1 << 40}


def _same(got, want, what):
    assert np.array_equal(got, want), "%s: streamed differs from resident (max |d| = %.3e)" % (
        what, float(np.abs(np.asarray(got) - np.asarray(want)).max()))


# ----------------------------------------------------------------------------- bit identity with the resident path
@pytest.mark.parametrize("N", [2, 3, 31, 64, 255, 256, 257, 1000, 1024, 1025])
def test_streamed_equals_resident_bit_for_bit(qfa, N):
    from quflow_amd.context import Context
    rng = np.random.default_rng(1000 + N)
    ctx = Context(N)
    try:
        r = Raw(ctx)
        r.check(r.lib.qf_basis_compute(ctx.handle))
        omega = rng.standard_normal(N * N)
        G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
        omc = rng.standard_normal(N * N) + 1j * rng.standard_normal(N * N)
        ns = sorted({n for n in _n_omegas(N) if n >= 1} | {min((e + 1) ** 4, N * N) for e in ELMAX})
        for n in ns:
            Nmax = band_limit(N, n)
            r.mode(0)
            want = (r.shr2mat(omega[:n]), r.mat2shr(G, n))
            for name, b in _budgets(N, Nmax).items():
                r.mode(b)
                what = "N=%d n_omega=%d slab=%s" % (N, n, name)
                _same(r.shr2mat(omega[:n]), want[0], "shr2mat " + what)
                _same(r.mat2shr(G, n), want[1], "mat2shr " + what)
        r.mode(0)
        want = (r.shc2mat(omc), r.mat2shc(G))
        for name, b in _budgets(N, N).items():
            r.mode(b)
            _same(r.shc2mat(omc), want[0], "shc2mat N=%d slab=%s" % (N, name))
            _same(r.mat2shc(G), want[1], "mat2shc N=%d slab=%s" % (N, name))
        # the NULL forms: the state, and coefficients left on the device for shr2fun / shr2mat
        for n in (N * N, (N // 2) ** 2 or 1):
            L = max(1, int(np.sqrt(n)))
            r.mode(0)
            want = r.null_forms(omega[:n], G, n, L)
            for name, b in _budgets(N, band_limit(N, n)).items():
                r.mode(b)
                got = r.null_forms(omega[:n], G, n, L)
                for k, what in enumerate(("shr2mat(state)", "mat2shr(state)", "mat2shr(NULL) -> shr2fun(NULL)",
                                          "mat2shr(NULL) -> shr2mat(NULL)")):
                    _same(got[k], want[k], "%s N=%d n_omega=%d slab=%s" % (what, N, n, name))
    finally:
        ctx.close()


def test_python_keyword_and_auto_choice(qfa):
    """streamed=True / False through the Python functions give the same bits; a fresh context in streamed mode needs no
    basis, and turning the mode off again refuses without one (the resident path's contract)."""
    from quflow_amd import _lib
    from quflow_amd import quantization as q
    from quflow_amd.context import Context
    N = 257
    rng = np.random.default_rng(5)
    omega = rng.standard_normal(N * N)
    G = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    for e in (-1, 4, 15):
        _same(q.mat2shr(G, elmax=e, streamed=True), q.mat2shr(G, elmax=e, streamed=False), "mat2shr elmax=%d" % e)
    _same(q.shr2mat(omega, N, streamed=True), q.shr2mat(omega, N, streamed=False), "shr2mat")
    _same(q.shc2mat(q.mat2shc(G, streamed=True), streamed=True), q.shc2mat(q.mat2shc(G, streamed=False), streamed=False),
          "mat2shc -> shc2mat")
    ctx = Context(64)
    try:
        r = Raw(ctx)
        r.mode(64 * 64 * 8)
        W = r.shr2mat(rng.standard_normal(64 * 64))
        assert np.count_nonzero(W) > 0
        r.mode(0)
        with pytest.raises(_lib.QuflowHipError, match="STATE"):
            r.shr2mat(np.ones(4))
        with pytest.raises(_lib.QuflowHipError, match="INVALID"):
            r.mode(-1)
        # a block larger than the budget is refused before anything is touched
        r.mode(64 * 64 * 8 - 8)
        r.upload(W)
        with pytest.raises(_lib.QuflowHipError, match="32768 bytes.*32760 bytes"):
            r.check(r.lib.qf_shr2mat(ctx.handle, r.ptr(np.ones(64 * 64)), ctypes.c_longlong(64 * 64), None))
        _same(r.download(), W, "the state after a refused call")
        r.mode(64 * 8 * 8)          # band limit 8: block 0 is 64 x 8
        r.check(r.lib.qf_shr2mat(ctx.handle, r.ptr(np.ones(64)), ctypes.c_longlong(64), None))
        r.mode(64 * 8 * 8 - 8)
        with pytest.raises(_lib.QuflowHipError, match="INVALID"):
            r.check(r.lib.qf_shr2mat(ctx.handle, r.ptr(np.ones(64)), ctypes.c_longlong(64), None))
    finally:
        ctx.close()


def test_streamed_guard_zones(qfa):
    """Under QUFLOW_HIP_DEBUG_GUARD=1, in a process of its own: streamed transforms with slabs filled to the last entry
    (budgets of exactly one block, and of the whole band) leave every guard zone intact, the slab's included."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, ctypes, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from quflow_amd import _lib, quantization as q\n"
        "from quflow_amd.context import Context, ptr\n"
        "lib = _lib.load()\n"
        "rng = np.random.default_rng(3)\n"
        "for N in (33, 300):\n"
        "    ctx = Context(N)\n"
        "    for n in (N * N, 17 ** 2, 5):\n"
        "        Nmax = N if n >= N * N else int(np.sqrt(n))\n"
        "        total = sum(8 * (N - m) * (Nmax - m) for m in range(Nmax))\n"
        "        for b in (8 * N * Nmax, total):\n"
        "            _lib.check(lib.qf_basis_stream(ctx.handle, ctypes.c_longlong(b)))\n"
        "            om = rng.standard_normal(n)\n"
        "            W = np.zeros((N, N), dtype=complex)\n"
        "            _lib.check(lib.qf_shr2mat(ctx.handle, ptr(om), ctypes.c_longlong(n), ptr(W)))\n"
        "            out = np.zeros(n)\n"
        "            _lib.check(lib.qf_mat2shr(ctx.handle, ptr(W), ptr(out), ctypes.c_longlong(n)))\n"
        "    full = sum(8 * (N - m) ** 2 for m in range(N))\n"
        "    for b in (8 * N * N, full):\n"
        "        _lib.check(lib.qf_basis_stream(ctx.handle, ctypes.c_longlong(b)))\n"
        "        G = rng.standard_normal((N, N)) + 0j\n"
        "        oc = np.zeros(N * N, dtype=complex)\n"
        "        _lib.check(lib.qf_mat2shc(ctx.handle, ptr(G), ptr(oc)))\n"
        "        _lib.check(lib.qf_shc2mat(ctx.handle, ptr(oc), ptr(W)))\n"
        "    ctx.close()\n"
        "a, d = ctypes.c_longlong(0), ctypes.c_longlong(0)\n"
        "t = ctypes.create_string_buffer(512)\n"
        "assert lib.qf_debug_guard_check(ctypes.byref(a), ctypes.byref(d), t, 512) == 0\n"
        "print((a.value, d.value, t.value.decode()))\n" % repo)
    env = dict(os.environ, QUFLOW_HIP_DEBUG_GUARD="1")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr)[-2000:]
    allocs, damaged, first = eval(res.stdout.strip().splitlines()[-1])
    assert allocs >= 8 and damaged == 0 and first == "", (allocs, damaged, first)


# ----------------------------------------------------------------------------- N = 4096 and 8192: no resident basis
def tridiagonal(N, m):
    """(diagonal, off-diagonal) of block m of the direct Laplacian: the oracle's compute_direct_laplacian entries for this
    block only, with its expressions and operation order (so the same bits), vectorised -- the oracle's double loop over
    all N^2 (m1, m2) pairs takes minutes at N = 8192."""
    s = (N - 1) / 2
    mv = np.linspace(-s, s, N)
    n = N - m
    m2, m1 = mv[:n], mv[m:]
    c1 = 2 * (s * (s + 1) - m1 * m2)
    d = np.where(np.abs(c1) > 1e-10, -c1, 0.0)
    a2, a1 = mv[:n - 1], mv[m:N - 1]
    c2 = -np.sqrt(s * (s + 1) - a1 * (a1 + 1)) * np.sqrt(s * (s + 1) - a2 * (a2 + 1))
    e = np.where(np.abs(c2) > 1e-10, -c2, 0.0)
    return d + 0.0, e + 0.0


def residual_ratio(N, m, B, cols):
    """||T_m b_j - lambda_j b_j||_inf / (eps ||T_m||_inf ||b_j||_2), lambda_j = -el (el + 1), el = m + j."""
    d, e = tridiagonal(N, m)
    TB = d[:, None] * B
    TB[:-1] += e[:, None] * B[1:]
    TB[1:] += e[:, None] * B[:-1]
    el = m + np.asarray(cols, dtype=np.float64)
    R = np.abs(TB + (el * (el + 1))[None, :] * B).max(axis=0)
    normT = np.abs(d).copy()
    normT[:-1] += np.abs(e)
    normT[1:] += np.abs(e)
    return R / (EPS * normT.max() * np.linalg.norm(B, axis=0))


def lapack_columns(N, m, cols):
    """Columns `cols` of the oracle's block m (compute_basis: eigh_tridiagonal, scaled by sqrt N, reversed so that
    column j <-> el = m + j, oriented by adjust_basis_orientation_), computed by index selection only.  The driver is the
    reference's own, MRRR (stemr): its twisted factorisations let the decaying tails of a vector underflow as the
    device's do, so the orientation rule, which reads the last entries, sees the same signs.  (Bisection + inverse
    iteration, scipy's default for a selection, leaves tails of ~1e-45 with arbitrary signs there.)"""
    d, e = tridiagonal(N, m)
    n = N - m
    cols = np.asarray(cols)
    out = np.empty((n, cols.shape[0]))
    # the small j (top of the spectrum) in one range, the others one by one: what keeps MRRR fast at n = 8192
    small = np.nonzero(cols <= 512)[0]
    runs = ([small] if small.shape[0] else []) + [np.array([k]) for k in np.nonzero(cols > 512)[0]]
    for run in runs:
        a, b = int(cols[run].min()), int(cols[run].max())
        v = eigh_tridiagonal(d, e, select="i", select_range=(n - 1 - b, n - 1 - a), lapack_driver="stemr")[1][:, ::-1]
        out[:, run] = v[:, cols[run] - a]
    out = out * np.sqrt(N)
    qo.adjust_basis_orientation_(out, m)       # column by column
    return out


def basis_bar(N, m, cols):
    """Per-column bound on max_k |b_dev[k] - b_lapack[k]|.

    Both sides are eigenvectors of the same fp64 matrix T_m computed with a residual of a few eps ||T_m|| ||b||
    (residual_ratio, checked separately); by Davis-Kahan the angle to the exact vector is at most residual / gap, with
    ||T_m|| ~ N^2 / 2 and, for el = m + j, the gap to the nearest other eigenvalue -el'(el'+1) of the block:
    2 el for el > m (to el - 1), 2 (m + 1) for el = m.  An entry of a column of norm sqrt N moves by at most the angle
    times sqrt N, and the two sides' errors add:  bar = 2 * C * eps * ||T_m||_inf * sqrt N / gap,  C = RESIDUAL_C = 8.
    (||T_m||_inf is 4.2e6 at N = 2048, 6.7e7 at 8192.)  At N = 2048 this is 3.4e-7 for el = 0, far above the 1e-12 N
    the 2048 tests hold with LAPACK's full blocks (observed errors sit well below the worst case); it falls like 1/el."""
    d, e = tridiagonal(N, m)
    normT = np.abs(d).copy()
    normT[:-1] += np.abs(e)
    normT[1:] += np.abs(e)
    el = m + np.asarray(cols, dtype=np.float64)
    gap = np.where(el > m, 2.0 * el, 2.0 * (m + 1))
    return 2 * 8.0 * EPS * normT.max() * np.sqrt(N) / gap


def check_large_columns(N, m, Bdev, cols, failures):
    """Residual, norm sqrt N, orientation and entries (basis_bar) of read-out columns of block m."""
    cols = np.asarray(cols)
    r = residual_ratio(N, m, Bdev, cols)
    for k in np.nonzero(r > 8.0)[0]:
        failures.append("residual of column j=%d (el=%d, m=%d): %.1f eps |T| |b|" % (cols[k], m + cols[k], m, r[k]))
    norm2 = (Bdev * Bdev).sum(axis=0)
    for k in np.nonzero(np.abs(norm2 - N) > 64 * EPS * N * N)[0]:
        failures.append("column j=%d (el=%d, m=%d): |b|^2 = %.17g, not N" % (cols[k], m + cols[k], m, norm2[k]))
    L = lapack_columns(N, m, cols)
    dots = np.einsum("ij,ij->j", Bdev, L)
    diff = np.abs(Bdev - L).max(axis=0)
    bar = basis_bar(N, m, cols)
    for k in np.nonzero((dots <= 0) | (diff > bar))[0]:
        failures.append("column j=%d (el=%d, m=%d): b_dev . b_lapack = %.3e, max|b_dev - b_lapack| = %.3e > %.3e"
                        % (cols[k], m + cols[k], m, dots[k], diff[k], bar[k]))
    return float((diff / bar).max())


LARGE = [4096, 8192]


@pytest.fixture(scope="module")
def large_ctx(qfa):
    """One context per large N in streamed mode at the default 4 GiB slab budget (no resident basis)."""
    from quflow_amd import quantization as q
    from quflow_amd.context import Context
    made = {}

    def get(N):
        if N not in made:
            for old in list(made):
                made.pop(old).ctx.close()
            made[N] = Raw(Context(N))
            made[N].mode(q.slab_bytes())
        return made[N]
    yield get
    for r in made.values():
        r.ctx.close()


def _read_columns(r, picks):
    """One shr2mat call with the single mode (el = m + j, +m) for every (m, j) of `picks` (at most one j per m): diagonal
    m of W holds 1j sgn B_m[:, j] (times 1/sqrt2 for m > 0).  Band-limited to the largest el.  Returns {m: column}."""
    N = r.N
    Nmax = max(m + j for m, j in picks) + 1
    omega = np.zeros(Nmax * Nmax)
    for m, j in picks:
        omega[_idx(m + j, m)] = 1.0
    W = r.shr2mat(omega)
    out = {}
    for m, j in picks:
        i = np.arange(N - m)
        up = W[i, i + m]
        assert np.all(up.real == 0.0)
        out[m] = _sgn(m) * up.imag * (1.0 if m == 0 else SQRT2)
        W[i, i + m] = 0.0
        W[i + m, i] = 0.0
    assert np.count_nonzero(W) == 0, "single modes wrote outside their diagonals"
    return out


@pytest.mark.parametrize("N", LARGE)
def test_streamed_columns_large(qfa, large_ctx, N):
    """Columns of sampled blocks read out through single-mode shr2mat: residual at -el(el+1), norm sqrt N, orientation and
    entries against LAPACK's columns to basis_bar.  Full-band calls read the last two columns of every sampled block at
    once; band-limited ones the columns at the tile and chunk edges of the small blocks and of block N/2."""
    r = large_ctx(N)
    ms = _sampled_ms(N)
    calls = [[(m, N - m - 1) for m in ms], [(m, N - m - 2) for m in ms if m < N - 1], [(N // 2, 0), (N // 2 + 1, 1)]]
    calls += [[(m, j) for m in ms if m <= 257] for j in (0, 1, 31, 32, 63, 64, 255, 256, 257)]
    cols = {m: {} for m in ms + [N // 2 + 1]}
    for picks in calls:
        for m, col in _read_columns(r, picks).items():
            cols[m][dict(picks)[m]] = col
    failures = []
    worst = 0.0
    for m, got in cols.items():
        js = sorted(got)
        worst = max(worst, check_large_columns(N, m, np.stack([got[j] for j in js], 1), js, failures))
    assert not failures, "\n".join(failures[:20])
    print("N=%d: %d columns read out; largest deviation from LAPACK %.2e of the bar"
          % (N, sum(len(c) for c in cols.values()), worst))


@pytest.mark.parametrize("N", LARGE)
def test_streamed_transforms_large(qfa, large_ctx, N):
    """shr2mat / mat2shr at full band and at lmax = 127 on sampled blocks against the extended-precision helpers on
    LAPACK's blocks (bar: the helper's rounding bound plus |dB| @ |x| with dB = basis_bar per column); the round trips
    mat2shr(shr2mat(omega)) ~ omega; nothing written past the band limit."""
    r = large_ctx(N)
    rng = np.random.default_rng(N + 1)
    full_ms = [N // 2, N - 2, N - 1]             # all of their columns: index selection keeps LAPACK affordable
    band_ms = [m for m in _sampled_ms(N) if m < 128]
    cache = {}

    def block(m):
        if m not in cache:
            cache[m] = lapack_columns(N, m, np.arange(N - m if m in full_ms else 128 - m))
        return cache[m]

    for n, ms in ((N * N, full_ms), (128 ** 2, band_ms)):
        Nmax = band_limit(N, n)
        omega = rng.standard_normal(n)
        W = r.shr2mat(omega)
        Wr, Wi, br, bi = ref_shr2mat(omega, N, block, ms)
        for m in ms:
            i = np.arange(N - m)
            els = np.arange(m, Nmax)
            xs = np.abs(omega[_idx(els, m)]) + (np.abs(omega[_idx(els, -m)]) if m else 0.0)
            extra = (basis_bar(N, m, els - m) * xs).sum()
            for a, b in ((i, i + m), (i + m, i)):
                assert_within(W.real[a, b], Wr[a, b], br[a, b] + extra, "shr2mat N=%d n=%d m=%d (real)" % (N, n, m))
                assert_within(W.imag[a, b], Wi[a, b], bi[a, b] + extra, "shr2mat N=%d n=%d m=%d (imag)" % (N, n, m))
        band = np.zeros((N, N), dtype=bool)
        for m in range(Nmax):
            i = np.arange(N - m)
            band[i, i + m] = band[i + m, i] = True
        assert np.count_nonzero(W[~band]) == 0
        out = r.mat2shr(W, n + 5)
        assert np.count_nonzero(out[Nmax * Nmax:]) == 0
        ref, bnd = ref_mat2shr(W, n, block, ms)
        for m in ms:
            els = np.arange(m, Nmax)
            d = np.abs(np.diagonal(W, -m))
            extra = SQRT2 * (basis_bar(N, m, els - m) * d.sum()) / N
            idx = np.concatenate([_idx(els, m), _idx(els, -m)]) if m else _idx(els, 0)
            bb = bnd.copy()
            bb[_idx(els, m)] += extra
            if m:
                bb[_idx(els, -m)] += extra
            assert_within(out[idx], ref[idx], bb[idx], "mat2shr N=%d n=%d m=%d" % (N, n, m))
        # round trip: two sums of <= N rounded terms each, and B^T B = N I to the columns' angle errors
        err = np.abs(out[:n] - omega).max() / np.abs(omega).max()
        assert err <= 1e-11 * N / 2048, "round trip N=%d n=%d: %.3e" % (N, n, err)
        print("N=%d n_omega=%d: round trip %.2e" % (N, n, err))


@pytest.mark.parametrize("N", LARGE)
def test_trajectory_large(qfa, N):
    """DeviceTrajectory at N = 4096 / 8192 (no resident basis): from_shr of random lmax = 127 data, a few steps, then
    shr() equals mat2shr(download(), streamed=True) and fun((N//2)^2) equals shr2fun of the same coefficients, bit for bit."""
    from quflow_amd import quantization as q
    from quflow_amd import transforms as T
    rng = np.random.default_rng(N + 2)
    omega = rng.standard_normal(128 ** 2) / (1.0 + np.floor(np.sqrt(np.arange(128 ** 2))))
    tr = qfa.DeviceTrajectory.from_shr(omega, N=N)
    try:
        W0 = tr.download()
        _same(W0, q.shr2mat(omega, N, streamed=True), "from_shr N=%d" % N)
        tr.advance(0.1 * qfa.hbar(N), 2)
        W = tr.download()
        assert np.abs(W - W0).max() > 0
        om = tr.shr()
        _same(om, q.mat2shr(W, streamed=True), "tr.shr() N=%d" % N)
        n = (N // 2) ** 2
        f = tr.fun(n_omega=n)
        _same(f, T.shr2fun(q.mat2shr(W, streamed=True)[:n]), "tr.fun((N//2)^2) N=%d" % N)
    finally:
        tr.ctx.close()
