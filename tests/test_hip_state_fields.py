"""Function-space output from the device (qf_state_fields; quflow_amd/csrc/sht.hip: k_sht_pack_fields,
k_sht_legendre_fields, k_sht_fourier_fields): DeviceTrajectory.fields, DeviceStackTrajectory.fields,
transforms.state_fields and Simulation(..., function_space=True).

The sizes: N = 33, 64, 65 put the bandwidth on, just past and far from the 64-row tile of the Fourier stage (a stack of
two fields at L = 33 or 65 has a tile that spans both); 257 is past the 256-ring block and the 256-degree chunk of the
Legendre stage; 130 has an odd half band (65); 3 is the smallest state (half band L = 1).
"""
import ctypes
import itertools
import pickle

import numpy as np
import pytest

import quflow_amd as qfa
from quflow_amd import _lib
from quflow_amd import transforms as T
from quflow_amd.context import Context, ptr
from quflow_amd.simulation import DirectoryStore, Simulation, solve

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
DEFAULT_PAIR = {'fun': np.float32, 'funL2': np.float32}
# every non-empty set of function-space qutypes the reference allows together (simulation.py:122-126)
SUBSETS = [tuple(q for q in pair if q) for pair in itertools.product(('fun', 'funhalf', None), ('funL2', 'funL2half', None))
           if any(pair)]


def skew(N, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    W = A - A.conj().T
    return np.ascontiguousarray(W / np.linalg.norm(W))


def composed(tr, N):
    """The four grids through the existing one-field API: tr.fun(n_omega, berezin), float64."""
    out = {}
    for q in T.FUNCTION_VARNAMES:
        n, berezin, _ = T.field_spec(q, N)
        out[q] = tr.fun(n, berezin)
    return out


def assert_fields(got, want64, qutypes, label):
    assert set(got) == set(qutypes), (label, set(got))
    for q, dt in qutypes.items():
        dt = np.dtype(dt)
        assert got[q].dtype == dt and got[q].shape == want64[q].shape, (label, q, got[q].dtype, got[q].shape)
        assert np.array_equal(got[q], want64[q].astype(dt)), (label, q, float(np.abs(got[q] - want64[q]).max()))


# ----------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("N", [3, 33, 64, 65, 130, 257])
def test_fields_have_the_bits_of_fun_and_astype(N):
    W, other = skew(N, N), skew(N, 1000 + N)
    tr = qfa.DeviceTrajectory(W)
    st = qfa.DeviceStackTrajectory(np.stack([other, W]))
    try:
        want = composed(tr, N)
        Wd = tr.download()
        for names in SUBSETS:
            kinds = [{q: F32 for q in names}, {q: F64 for q in names}]
            if len(names) == 2:
                kinds.append({names[0]: F64, names[1]: F32})       # (both dtypes in one stacked call)
            for qutypes in kinds:
                label = "N=%d %s" % (N, {q: str(d) for q, d in qutypes.items()})
                assert_fields(tr.fields(qutypes), want, qutypes, "tr.fields " + label)
                assert_fields(T.state_fields(Wd, qutypes), want, qutypes, "state_fields " + label)
                assert_fields(st.fields(1, qutypes), want, qutypes, "stack member 1 " + label)
        # a (k,N,N) host stack, member by member
        both = T.state_fields(np.stack([other, W]), DEFAULT_PAIR)
        assert both['fun'].shape == (2, N, 2 * N - 1) and both['fun'].dtype == F32
        assert np.array_equal(both['fun'][1], want['fun'].astype(F32))
        assert np.array_equal(both['funL2'][0], st.fields(0, DEFAULT_PAIR)['funL2'])
    finally:
        tr.ctx.close()
        st.ctx.close()


@pytest.mark.parametrize("N", [3, 33, 64, 65, 130, 257])
def test_three_and_four_fields_of_one_bandwidth_through_the_c_abi(N):
    """The qutypes' rules never put more than two fields at one bandwidth; the entry point takes up to four (here the
    same two grids in both dtypes, then three of them, at the full and at the half band in one call of eight fields)."""
    tr = qfa.DeviceTrajectory(skew(N, N))
    try:
        want = composed(tr, N)
        full, half = N * N, (N // 2) ** 2
        L2 = T._bandwidth(half, -1)
        specs = [(full, 1, 0, 'fun'), (full, 0, 1, 'funL2'), (full, 1, 1, 'fun'), (full, 0, 0, 'funL2'),
                 (half, 0, 0, 'funL2half'), (half, 1, 1, 'funhalf'), (half, 0, 1, 'funL2half'), (half, 1, 0, 'funhalf')]
        for use in (specs, specs[:3] + specs[4:7]):
            arr = (_lib.Field * len(use))(*[_lib.Field(n, b, d) for n, b, d, _ in use])
            outs = [np.empty((N, 2 * N - 1) if n == full else (L2, 2 * L2 - 1), dtype=F32 if d else F64) for n, b, d, _ in use]
            ptrs = (ctypes.c_void_p * len(use))(*[o.ctypes.data for o in outs])
            _lib.check(tr.ctx._lib.qf_state_fields(tr.ctx.handle, None, len(use), arr, ptrs))
            for (n, b, d, q), o in zip(use, outs):
                assert np.array_equal(o, want[q].astype(o.dtype)), (N, len(use), n, b, d)
    finally:
        tr.ctx.close()


@pytest.mark.parametrize("N", [33, 130])
def test_an_shr_row_shares_the_sweep_of_the_fields(N):
    """fields_and_shr: the coefficients the sweep of a full-band field left on the device are tr.shr(), bit for bit; with
    half-band fields alone they are swept on their own.  qf_shr_held refuses more than the device copy holds."""
    tr = qfa.DeviceTrajectory(skew(N, 21))
    try:
        omega = tr.shr()
        want = composed(tr, N)
        for qutypes in ({'fun': F32, 'funL2half': F64}, {'funL2': F64}, {'funhalf': F32}):
            got, om = tr.fields_and_shr(qutypes)
            assert_fields(got, want, qutypes, "fields_and_shr N=%d %s" % (N, sorted(qutypes)))
            assert np.array_equal(om, omega), sorted(qutypes)
        tr.fields({'funhalf': F32})                     # (the device copy now holds (N//2)^2 coefficients)
        buf = np.zeros(N * N)
        assert tr.ctx._lib.qf_shr_held(tr.ctx.handle, ptr(buf), ctypes.c_longlong(N * N)) == 4          # QF_ERR_STATE
        half = (N // 2) ** 2
        assert tr.ctx._lib.qf_shr_held(tr.ctx.handle, ptr(buf), ctypes.c_longlong(half)) == 0
        assert np.array_equal(buf[:half], omega[:half]) and not buf[half:].any()
    finally:
        tr.ctx.close()


def test_streamed_basis_sweeps_once_per_bandwidth(monkeypatch):
    """With a streamed basis (forced here at a small N that no other test caches a basis for) the call sweeps once per
    bandwidth: two bandwidths in one call have the bits of tr.fun under the same mode, and fields_and_shr falls back to
    shr() when the last sweep was the half band, but copies the coefficients out when it was the full one."""
    from quflow_amd import quantization
    N = 38
    monkeypatch.setenv("QUFLOW_HIP_BASIS_RESIDENT_MB", "0")
    assert quantization.use_streamed(N)
    tr = qfa.DeviceTrajectory(skew(N, 38))
    try:
        want = composed(tr, N)
        omega = tr.shr()
        for qutypes in ({'fun': F64, 'funL2half': F32}, {'funhalf': F64, 'funL2': F32}, {'funhalf': F32, 'funL2half': F64}):
            assert_fields(tr.fields(qutypes), want, qutypes, "streamed N=%d %s" % (N, sorted(qutypes)))
            got, om = tr.fields_and_shr(qutypes)
            assert_fields(got, want, qutypes, "streamed fields_and_shr %s" % sorted(qutypes))
            assert np.array_equal(om, omega), sorted(qutypes)
        # the half band swept last: the device copy holds (N//2)^2 coefficients and the full vector is refused
        tr.fields({'fun': F64, 'funL2half': F32})
        buf = np.zeros(N * N)
        assert tr.ctx._lib.qf_shr_held(tr.ctx.handle, ptr(buf), ctypes.c_longlong(N * N)) == 4          # QF_ERR_STATE
    finally:
        tr.ctx.close()


# ----------------------------------------------------------------------------- 2. independent check
@pytest.mark.parametrize("N, names", [(257, ('fun', 'funL2')), (130, ('funhalf', 'funL2half'))])
def test_fields_against_the_long_double_evaluator(N, names):
    """The float64 fields to the bar of tests/test_hip_sht_large.py on the coefficients tr.shr() returns; the float32
    fields to the same bar plus 2^-24 |ref| per point, the rounding of the cast."""
    from test_hip_sht_large import EPS, _check, _rings, _scale_l
    from test_transforms_host import legendre_sums, synth_rings
    tr = qfa.DeviceTrajectory(skew(N, 7 * N))
    try:
        n = T.field_spec(names[0], N)[0]
        omega = tr.shr(n)
        f64 = tr.fields({q: F64 for q in names})
        f32 = tr.fields({q: F32 for q in names})
    finally:
        tr.ctx.close()
    L = T._bandwidth(n, -1)
    rings = _rings(L)
    for q in names:
        berezin = T.field_spec(q, N)[1]
        Gp, Gm, scale = legendre_sums(T.shr2shc(omega), L, rings, scale_l=_scale_l(L, berezin))
        _check(f64[q][rings], Gp, Gm, scale, L, True, "fields N=%d %s float64" % (N, q))
        ref, err_ref = synth_rings(Gp, Gm, L, True)
        bar = (32 * L * EPS * scale + err_ref)[:, None] + 1e-300 + 2.0 ** -24 * np.abs(ref)
        err = np.abs(f32[q][rings].astype(np.float64) - ref)
        print("fields N=%d %s float32: max err %.3e  err/bar %.3e" % (N, q, float(err.max()), float((err / bar).max())))
        assert not (err > bar).any(), (q, float((err / bar).max()))


# ----------------------------------------------------------------------------- 3. the run is untouched
@pytest.mark.parametrize("N, hooked", [(65, False), (64, True)], ids=["unforced-65", "forced-64"])
def test_a_fields_call_leaves_the_run_untouched(N, hooked):
    W = skew(N, 3)
    dt = 0.25 * qfa.hbar(N)

    def make():
        if not hooked:
            return qfa.DeviceTrajectory(W)
        return qfa.DeviceTrajectory(W, forcing=qfa.AffineForcing(F0=1e-3 * skew(N, 4), a_W=-0.05, a_P=0.02),
                                    strang_splitting=qfa.ViscDampStep(nu=1e-3, alpha=0.01))
    runs = []
    for with_fields in (False, True):
        tr = make()
        try:
            s1 = tr.advance(dt, 5)
            if with_fields:
                f = tr.fields(DEFAULT_PAIR)
                assert f['fun'].shape == (N, 2 * N - 1)
            s2 = tr.advance(dt, 5)
            runs.append((tr.download(), s1, s2))
        finally:
            tr.ctx.close()
    assert np.array_equal(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]


# ----------------------------------------------------------------------------- 4. shared scratch
def _other_transforms(ctx):
    """qf_shr2fun at L = 200 and qf_fun2shr at L = 40 on `ctx`, the buffers of ctx->sht shared with the fields."""
    lib = ctx._lib
    rng = np.random.default_rng(11)
    om = rng.standard_normal(200 * 200)
    f = np.empty((200, 399))
    _lib.check(lib.qf_shr2fun(ctx.handle, ptr(om), ctypes.c_longlong(om.size), 200, 1, ptr(f)))
    g = np.ascontiguousarray(rng.standard_normal((40, 79)))
    back = np.empty(1600)
    _lib.check(lib.qf_fun2shr(ctx.handle, ptr(g), 40, 1, ptr(back)))
    return f, back


def test_fields_interleave_with_other_transforms_on_one_context():
    N = 130
    q = {'fun': F64, 'funL2half': F32}          # L = 130 and L = 65: two syntheses in one call
    tr = qfa.DeviceTrajectory(skew(N, 5))
    fresh = Context(N, tr.ctx.device)
    try:
        first = tr.fields(q)
        assert first['fun'].shape == (130, 259) and first['funL2half'].shape == (65, 129)
        f, back = _other_transforms(tr.ctx)
        second = tr.fields(q)
        f0, back0 = _other_transforms(fresh)
    finally:
        tr.ctx.close()
        fresh.close()
    for k in q:
        assert np.array_equal(first[k], second[k]), k
    assert np.array_equal(f, f0) and np.array_equal(back, back0)


# ----------------------------------------------------------------------------- 5. records
def _run_record(path, W, qutypes, function_space, **kw):
    sim = Simulation(str(path), overwrite=True, state=W, qutypes=qutypes, function_space=function_space)
    solve(W.copy(), stepsize=0.1, steps=6, steps_out=2, callback=sim, progress_bar=False, **kw)
    return sim


def test_solve_writes_the_default_pair_resident_and_on_the_host_path(tmp_path):
    N = 33
    W = skew(N, 8)
    qutypes = {'mat': None, 'fun': np.float32, 'funL2': np.float32}
    res = _run_record(tmp_path / "res", W, qutypes, True)
    host = _run_record(tmp_path / "host", W, qutypes, True, resident=False, integrator=qfa.isomp)
    plain = _run_record(tmp_path / "plain", W, {'mat': None}, False)
    assert set(res.fieldnames) == set(plain.fieldnames) | {'fun', 'funL2'}
    for name in res.fieldnames:
        assert np.array_equal(res[name], host[name]), name
    for name in plain.fieldnames:
        assert np.array_equal(res[name], plain[name]), name
    assert res['fun'].shape == (4, 33, 65) and res['fun'].dtype == F32
    assert res['funL2'].shape == (4, 33, 65) and res['funL2'].dtype == F32
    for i in range(4):
        om = qfa.mat2shr(res['mat', i])
        assert np.array_equal(res['fun', i], qfa.shr2fun(om).astype(F32)), i
        assert np.array_equal(res['funL2', i], qfa.shr2fun(om, berezin=False).astype(F32)), i


def test_solve_writes_funhalf_next_to_shr(tmp_path):
    N, L = 34, 17
    W = skew(N, 9)
    qutypes = {'funhalf': np.float64, 'shr': None}
    res = _run_record(tmp_path / "res", W, qutypes, True)
    host = _run_record(tmp_path / "host", W, qutypes, True, resident=False, integrator=qfa.isomp)
    assert 'funhalf' not in res.fieldnames and res['fun'].shape == (4, L, 2 * L - 1) and res['fun'].dtype == F64
    assert res['shr'].shape == (4, N * N)
    for name in res.fieldnames:
        assert np.array_equal(res[name], host[name]), name
    for i in range(4):
        assert np.array_equal(res['fun', i], qfa.shr2fun(res['shr', i][:L * L])), i


def test_solve_writes_fun_next_to_shr_from_one_sweep(tmp_path):
    N = 33
    W = skew(N, 14)
    qutypes = {'shr': None, 'fun': np.float32}
    res = _run_record(tmp_path / "res", W, qutypes, True)
    host = _run_record(tmp_path / "host", W, qutypes, True, resident=False, integrator=qfa.isomp)
    only = _run_record(tmp_path / "only", W, {'shr': None}, False)
    for name in res.fieldnames:
        assert np.array_equal(res[name], host[name]), name
    assert np.array_equal(res['shr'], only['shr'])
    for i in range(4):
        assert np.array_equal(res['fun', i], qfa.shr2fun(res['shr', i]).astype(F32)), i


def test_solve_writes_the_rows_of_a_stack(tmp_path):
    N, L = 34, 17
    W = np.stack([skew(N, 10), skew(N, 11)])
    qutypes = {'mat': None, 'funhalf': np.float64, 'funL2': np.float32}
    res = _run_record(tmp_path / "res", W, qutypes, True)
    host = _run_record(tmp_path / "host", W, qutypes, True, resident=False, integrator=qfa.isomp)
    assert res['fun'].shape == (4, 2, L, 2 * L - 1) and res['funL2'].shape == (4, 2, N, 2 * N - 1)
    for name in res.fieldnames:
        assert np.array_equal(res[name], host[name]), name
    for i in (0, 3):
        for j in range(2):
            om = qfa.mat2shr(res['mat', i, j])
            assert np.array_equal(res['fun', i, j], qfa.shr2fun(om[:L * L])), (i, j)
            assert np.array_equal(res['funL2', i, j], qfa.shr2fun(om, berezin=False).astype(F32)), (i, j)


# ----------------------------------------------------------------------------- 6. a file with the reference's defaults
def test_append_to_a_record_with_the_reference_default_qutypes(tmp_path):
    """The record of tests/test_h5_interop.py:166-182 (one row of mat, fun, funL2, time, step under the reference's default
    qutypes), built through the directory store: with the keyword a row is appended, without it the call still raises."""
    N = 8
    W = skew(N, 12)
    path = str(tmp_path / "defaults")
    store = DirectoryStore(path, True)
    store.set_attr("attrs", "qutypes", pickle.dumps({'mat': None, 'fun': np.float32, 'funL2': np.float32}))
    store.set_attr("attrs", "loggers", pickle.dumps({}))
    store.set_attr("attrs", "N", N)
    store.create("mat", W)
    for name in ("fun", "funL2"):
        store.create(name, np.zeros((N, 2 * N - 1), dtype=np.float32))
    store.create("time", np.float64(0.0))
    store.create("step", np.int64(0))
    closed = Simulation(path)
    with pytest.raises(NotImplementedError, match="function_space"):
        closed(W=W, delta_time=0.1, delta_steps=1)
    assert closed.fieldnames['mat'][0] == (1, N, N) and closed.fieldnames['fun'][0] == (1, N, 2 * N - 1)
    sim = Simulation(path, function_space=True)
    sim(W=W, delta_time=0.1, delta_steps=1)
    for name, berezin in (("fun", True), ("funL2", False)):
        assert sim.fieldnames[name] == ((2, N, 2 * N - 1), F32)
        assert np.array_equal(sim[name, 1], qfa.shr2fun(qfa.mat2shr(W), berezin=berezin).astype(F32))
    assert sim.fieldnames['mat'][0] == (2, N, N) and sim['step', -1] == 1


# ----------------------------------------------------------------------------- 7. argument rules of the C entry point
def test_bad_arguments_are_refused_before_any_launch():
    N = 16
    tr = qfa.DeviceTrajectory(skew(N, 13))
    try:
        tr._need_basis()
        before = tr.fields(DEFAULT_PAIR)
        W0 = tr.download()
        lib, h = tr.ctx._lib, tr.ctx.handle
        grids = [np.empty((N, 2 * N - 1)) for _ in range(5)]

        def call(specs, outs):
            arr = (_lib.Field * len(specs))(*[_lib.Field(*s) for s in specs])
            ptrs = (ctypes.c_void_p * len(specs))(*[None if o is None else o.ctypes.data for o in outs])
            return lib.qf_state_fields(h, None, len(specs), arr, ptrs)

        bad = {"five fields of one L": ([(N * N, 1, 0)] * 5, grids),
               "dtype 2": ([(N * N, 1, 2)], grids[:1]),
               "n_omega 0": ([(0, 1, 0)], grids[:1]),
               "null grid": ([(N * N, 1, 0), (N * N, 0, 0)], [grids[0], None]),
               "L above N": ([((N + 1) ** 2, 1, 0)], grids[:1])}
        for label, (specs, outs) in bad.items():
            assert call(specs, outs) == 1, label                                   # QF_ERR_INVALID
            assert b"qf_state_fields" in lib.qf_last_error(), label
        assert b"field 1" in (call(*bad["null grid"]) and lib.qf_last_error())
        assert lib.qf_state_fields(h, None, 0, None, None) == 1 and lib.qf_state_fields(h, None, 9, None, None) == 1
        assert np.array_equal(tr.download(), W0)
        after = tr.fields(DEFAULT_PAIR)
        for q in DEFAULT_PAIR:
            assert np.array_equal(before[q], after[q]), q
    finally:
        tr.ctx.close()
