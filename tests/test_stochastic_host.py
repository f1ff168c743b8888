"""Host-side checks of the stochastic band-limited forcing (qf_set_stochastic_forcing, k_stoch_draw,
quflow_amd.StochasticForcing): what can be said without a GPU -- the generator's known answers and the uniform mapping on the
numpy mirror, the moments of draw_host, what a coefficient depends on, the constructor's rules, pickling with the counter,
what simulation._resident_kind makes of a stochastic run, the routes that refuse, the expected energy injection against a
sample, the code generator's record of the new kernel and the ctypes prototypes of the new entry points."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from conftest import REPO

NEW_SYMBOLS = ("qf_set_stochastic_forcing", "qf_stochastic_tell", "qf_stochastic_seek", "qf_stochastic_pattern")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from quflow_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def qfa():
    import quflow_amd
    return quflow_amd


def skew(N, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))
    return A - A.conj().T


def words(x):
    return " ".join("%08x" % int(v) for v in x)


# ----------------------------------------------------------------------------- the generator
KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(qfa, counter, key, want):
    assert words(qfa.laplacian.philox4x32_10(counter, key)) == want


def test_philox_is_elementwise_on_arrays(qfa):
    """The mirror runs on arrays of counters: every lane equals the scalar call."""
    b = np.arange(0, 5000, 7, dtype=np.uint64)
    x = qfa.laplacian.philox4x32_10((5, 1, b, 0), (0xa4093822, 0x299f31d0))
    for i in (0, 1, 17, len(b) - 1):
        one = qfa.laplacian.philox4x32_10((5, 1, int(b[i]), 0), (0xa4093822, 0x299f31d0))
        assert [int(w[i]) for w in x] == [int(w) for w in one]


def test_uniform_mapping_at_the_word_extremes(qfa):
    u, v = qfa.laplacian.philox_uniforms(0, 0, 0, 0)
    assert u == 2.0 ** -53 and v == 0.0
    f = 0xffffffff
    u, v = qfa.laplacian.philox_uniforms(f, f, f, f)
    assert u == 1.0 and v == 1.0 - 2.0 ** -53
    assert np.sqrt(-2.0 * np.log(u)) == 0.0               # r = 0: the largest uniform gives the zero normal, never a NaN
    assert np.isfinite(np.sqrt(-2.0 * np.log(2.0 ** -53)))


def test_moments_of_draw_host(qfa):
    """4,096 steps of the band [1, 3]: n = 61,440 unit normals (sigma = 1, scaled back by sqrt(dt)); 5-sigma bounds from n."""
    dt = 0.37
    sf = qfa.StochasticForcing(1, 3, 1.0, seed=20261018)
    x = np.concatenate([sf.draw_host(n, dt)[1:] for n in range(4096)]) * np.sqrt(dt)
    n = x.size
    assert n == 61440
    mean, var = float(x.mean()), float(x.var())
    print("mean %.3e (bound %.3e), var - 1 %.3e (bound %.3e)" % (mean, 5 / np.sqrt(n), var - 1, 5 * np.sqrt(2.0 / n)))
    assert abs(mean) <= 5 / np.sqrt(n)
    assert abs(var - 1.0) <= 5 * np.sqrt(2.0 / n)
    # cosine and sine halves separately, and no correlation between the pair of a block
    a, b = x[1::2], x[0::2]        # (q odd / even alternate along the array: band entries start at q = 1)
    assert abs(float(a.mean())) <= 5 / np.sqrt(a.size) and abs(float(b.mean())) <= 5 / np.sqrt(b.size)


def test_a_coefficient_depends_on_seed_step_l_m_only(qfa):
    dt = 0.25
    a = qfa.StochasticForcing(2, 5, 0.5, seed=7)
    wide = qfa.StochasticForcing(1, 9, 0.5, seed=7)
    oa, ow = a.draw_host(3, dt), wide.draw_host(3, dt)
    assert oa.shape == (36,) and ow.shape == (100,)
    assert np.array_equal(oa[4:36], ow[4:36])              # another band: the shared entries are the same numbers
    assert not np.any(oa[:4]) and np.all(oa[4:] != 0)      # zeros outside the band, exactly
    # another amplitude rescales (sigma * inv) and nothing else: xi is the same
    b = qfa.StochasticForcing(2, 5, 2.0, seed=7)
    assert np.array_equal(b.draw_host(3, dt)[4:] / (2.0 * 2.0), oa[4:] / (0.5 * 2.0))      # (powers of two: exact)
    # one sigma per l
    per_l = qfa.StochasticForcing(2, 5, [0.5, 0.0, 0.5, 1.0], seed=7)
    oc = per_l.draw_host(3, dt)
    assert np.array_equal(oc[4:9], oa[4:9]) and not np.any(oc[9:16]) and np.array_equal(oc[25:36], 2.0 * oa[25:36])
    # another seed, another step: other numbers
    assert not np.array_equal(qfa.StochasticForcing(2, 5, 0.5, seed=8).draw_host(3, dt), oa)
    assert not np.array_equal(a.draw_host(4, dt), oa)
    assert not np.array_equal(a.draw_host(3 + 2 ** 32, dt), oa)       # the counter's high word counts
    assert not np.array_equal(qfa.StochasticForcing(2, 5, 0.5, seed=7 + 2 ** 32).draw_host(3, dt), oa)
    # `.step` does not enter a draw
    a.step = 99
    assert np.array_equal(a.draw_host(3, dt), oa)


# ----------------------------------------------------------------------------- the constructor
def test_constructor_keeps_what_it_is_given(qfa):
    sf = qfa.StochasticForcing(2, 4, [1.0, 2.0, 3.0], seed=5, a_W=-0.01, a_P=0.5, a_lap=1e-4, step=11)
    assert (sf.l_min, sf.l_max, sf.seed, sf.step) == (2, 4, 5, 11)
    assert (sf.a_W, sf.a_P, sf.a_lap) == (-0.01, 0.5, 1e-4)
    assert sf.sigma.dtype == np.float64 and sf.sigma.tolist() == [1.0, 2.0, 3.0] and not sf.sigma.flags.writeable
    assert qfa.StochasticForcing(2, 4, 0.5, 0).sigma.tolist() == [0.5, 0.5, 0.5]
    assert qfa.StochasticForcing(np.int64(1), np.int32(1), np.float32(2), np.uint64(3)).sigma.tolist() == [2.0]
    sf.check_size(5)
    with pytest.raises(ValueError, match="l_max=4"):
        sf.check_size(4)


def test_constructor_rules(qfa):
    S = qfa.StochasticForcing
    for bad in ((0, 3), (-1, 3), (4, 3), (1, 8192)):
        with pytest.raises(ValueError, match="l_m"):
            S(bad[0], bad[1], 1.0, 0)
    for bad in (1.0, "1", None, True):
        with pytest.raises(TypeError, match="l_min"):
            S(bad, 3, 1.0, 0)
        with pytest.raises(TypeError, match="l_max"):
            S(1, bad, 1.0, 0)
    for bad in ([1.0, 2.0], np.ones((3, 1)), np.ones(4)):
        with pytest.raises(ValueError, match="sigma"):
            S(1, 3, bad, 0)
    for bad in (-1.0, np.nan, np.inf, [1.0, -0.5, 1.0], [1.0, np.nan, 1.0]):
        with pytest.raises(ValueError, match="sigma"):
            S(1, 3, bad, 0)
    for bad in ("1.0", 1j, None, True):
        with pytest.raises(TypeError, match="sigma"):
            S(1, 3, bad, 0)
    for name in ("seed", "step"):
        for bad in (1.5, "3", None, True):
            with pytest.raises(TypeError, match=name):
                S(1, 3, 1.0, **{"seed": 0, name: bad})
        for bad in (-1, 2 ** 64):
            with pytest.raises(ValueError, match=name):
                S(1, 3, 1.0, **{"seed": 0, name: bad})
    assert S(1, 3, 1.0, seed=2 ** 64 - 1, step=2 ** 64 - 1).seed == 2 ** 64 - 1
    for name in ("a_W", "a_P", "a_lap"):
        for bad in (1j, "1.0", None, [1.0]):
            with pytest.raises(TypeError, match=name):
                S(1, 3, 1.0, 0, **{name: bad})
        for bad in (np.nan, np.inf):
            with pytest.raises(ValueError, match=name):
                S(1, 3, 1.0, 0, **{name: bad})
    sf = S(1, 3, 1.0, 0)
    for bad in (0.0, -0.1, np.inf, np.nan):
        with pytest.raises(ValueError, match="dt"):
            sf.draw_host(0, bad)
    with pytest.raises(ValueError, match="n "):
        sf.draw_host(-1, 0.1)


def test_pickle_round_trip_with_the_counter(qfa):
    sf = qfa.StochasticForcing(2, 5, [0.5, 0.0, 0.5, 1.0], seed=2 ** 40 + 3, a_W=-0.02, a_lap=1e-5, step=4)
    sf.step = 2 ** 33 + 17                   # what a run leaves
    g = pickle.loads(pickle.dumps(sf))
    assert type(g) is qfa.StochasticForcing
    assert (g.l_min, g.l_max, g.seed, g.step, g.a_W, g.a_P, g.a_lap) == (2, 5, 2 ** 40 + 3, 2 ** 33 + 17, -0.02, 0.0, 1e-5)
    assert np.array_equal(g.sigma, sf.sigma)
    assert np.array_equal(g.draw_host(g.step, 0.1), sf.draw_host(sf.step, 0.1))


# ----------------------------------------------------------------------------- what solve keeps on the device, who refuses
def test_resident_kind_of_stochastic_runs(qfa):
    from quflow_amd import simulation
    kind = simulation._resident_kind
    N = 8
    W = skew(N, 5)
    sf = qfa.StochasticForcing(2, 5, 0.1, seed=1, a_W=-0.01)
    v = qfa.ViscDampStep(nu=1e-4, alpha=0.01)
    H = qfa.TridiagonalHamiltonian(np.ones((N, N, 2)), offset=qfa.coriolis(N, 1.0))
    base = {"hamiltonian": qfa.solve_poisson, "time": 0.0, "stats": {}}
    for isomp in (qfa.isomp, qfa.isomp_fixedpoint):
        assert kind(isomp, dict(base, forcing=sf), W) == 'single'
        assert kind(isomp, dict(base, forcing=sf, strang_splitting=v), W) == 'single'
        assert kind(isomp, dict(base, forcing=sf, strang_splitting=v, hamiltonian=H), W) == 'single'
        assert kind(isomp, dict(base, forcing=sf, compsum=True), W) is None
        assert kind(isomp, dict(base, forcing=sf, callback=lambda W, dW: None), W) is None
        assert kind(isomp, dict(base, forcing=sf, strang_splitting=lambda h, W: W), W) is None
        assert kind(isomp, dict(base, forcing=sf), np.stack([W, W])) is None
        assert kind(isomp, dict(base, forcing=sf), W.astype(np.complex64)) is None
    assert kind(qfa.rk4, dict(base, forcing=sf), W) is None
    try:
        qfa.integrators.select_skewherm(False)
        assert kind(qfa.isomp, dict(base, forcing=sf), W) is None
    finally:
        qfa.integrators.select_skewherm(True)


def test_routes_that_do_not_follow_raise_before_they_touch_a_device(qfa):
    N = 8
    W = skew(N, 6)
    sf = qfa.StochasticForcing(2, 5, 0.1, seed=1)
    dt = 0.01
    routes = {
        "stack": lambda: qfa.isomp(np.stack([W, W]), dt, steps=1, forcing=sf),
        "magmp": lambda: qfa.magmp(np.stack([W, W]), dt, steps=1, forcing=sf),
        "complex64": lambda: qfa.isomp(W.astype(np.complex64), dt, steps=1, forcing=sf),
        "euler": lambda: qfa.euler(W.copy(), dt, steps=1, forcing=sf),
        "heun": lambda: qfa.heun(W.copy(), dt, steps=1, forcing=sf),
        "rk4": lambda: qfa.rk4(W.copy(), dt, steps=1, forcing=sf),
        "rk4 stack": lambda: qfa.rk4(np.stack([W, W]), dt, steps=1, forcing=sf),
        "isomp_simple": lambda: qfa.isomp_simple(W.copy(), dt, steps=1, forcing=sf),
        "isomp_quasinewton": lambda: qfa.isomp_quasinewton(W.copy(), dt, steps=1, forcing=sf),
        "as a callable": lambda: sf(W, W),
    }
    for name, call in routes.items():
        with pytest.raises(NotImplementedError, match="DeviceTrajectory"):
            call()
    try:
        qfa.integrators.select_skewherm(False)
        with pytest.raises(NotImplementedError, match="select_skewherm"):
            qfa.isomp(W.copy(), dt, steps=1, forcing=sf)
    finally:
        qfa.integrators.select_skewherm(True)
    assert sf.step == 0
    # a band the state cannot carry
    with pytest.raises(ValueError, match="l_max=9"):
        qfa.isomp(W.copy(), dt, steps=1, forcing=qfa.StochasticForcing(2, 9, 0.1, seed=1))
    with pytest.raises(ValueError, match="l_max=9"):
        qfa.DeviceTrajectory(W, forcing=qfa.StochasticForcing(2, 9, 0.1, seed=1))
    with pytest.raises(ValueError, match="l_max=9"):
        qfa.StochasticForcing(2, 9, 0.1, seed=1).as_callable(dt, N)


# ----------------------------------------------------------------------------- injection rates
def test_energy_rate_against_a_sample(qfa, built, monkeypatch):
    """E(dt F0_n) / dt over 1,500 steps at N = 8, band [1, 3] with one sigma per l: F0_n from draw_host and the unit-norm_L2
    basis elements elmr2mat (the basis from the CPU oracle), E = energy_euler of the CPU oracle.  The sample mean lies within
    5 standard errors -- the sample's own -- of energy_rate(); the same for the enstrophy."""
    from oracle import quantization_oracle as qo, isomp_oracle as io
    from quflow_amd import quantization
    N, dt, M = 8, 0.05, 1500
    monkeypatch.setitem(quantization._basis_cache, (N, np.dtype(np.float64)), np.ascontiguousarray(qo.compute_basis(N)))
    sf = qfa.StochasticForcing(1, 3, [0.7, 0.0, 1.3], seed=99)
    T = {}
    for el in range(1, 4):
        for m in range(-el, el + 1):
            T[el * el + el + m] = qfa.elmr2mat(el, m, N).toarray()
            assert abs(qfa.norm_L2(T[el * el + el + m]) - 1.0) <= 1e-13       # the normalisation the formulas rest on
    e, s = np.empty(M), np.empty(M)
    for n in range(M):
        om = sf.draw_host(n, dt)
        F0 = sum(om[q] * Tq for q, Tq in T.items())
        e[n] = io.energy_euler(np.ascontiguousarray(dt * F0)) / dt
        s[n] = io.enstrophy(np.ascontiguousarray(dt * F0)) / dt
    for name, x, want in (("energy", e, sf.energy_rate()), ("enstrophy", s, sf.enstrophy_rate())):
        bound = 5 * x.std(ddof=1) / np.sqrt(M)
        print("%s: sample mean %.6f, expected %.6f, 5 standard errors %.6f" % (name, x.mean(), want, bound))
        assert abs(x.mean() - want) <= bound
    assert sf.energy_rate() == pytest.approx(0.5 * (3 * 0.49 / 2 + 7 * 1.69 / 12), rel=1e-14)
    assert sf.enstrophy_rate() == pytest.approx(0.5 * (3 * 0.49 + 7 * 1.69), rel=1e-14)


# ----------------------------------------------------------------------------- the build's records and the ABI
def test_draw_kernel_in_the_build_records(built):
    from test_abi_and_host import kernel_resources
    res = kernel_resources()
    assert "k_stoch_draw" in res, sorted(k for k in res if "stoch" in k)
    r = res["k_stoch_draw"]
    assert r["unit"] == "stochastic.res", r
    assert r["scratch"] == 0 and not r["dynamic_stack"] and r["lds"] == 0, r
    # the band transform it feeds: the slab instantiation of the real matvec is still there, in the transforms' unit
    assert res["k_block_matvec<0, true>"]["unit"] == "quantization.res"


def test_new_symbols_resolve_with_their_signatures(built):
    lib = built.load()
    header = open(os.path.join(REPO, "include", "quflow_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in built.SIGNATURES, name
        fn = getattr(lib, name)
        res, args = built.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args), name
        assert re.search(r"\bint %s\(qf_ctx \*ctx" % name, header), name
    assert built.SIGNATURES["qf_set_stochastic_forcing"][1] == [
        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_ulonglong, ctypes.c_double,
        ctypes.c_double, ctypes.c_double, ctypes.c_longlong]
    assert built.SIGNATURES["qf_stochastic_tell"][1] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
    assert built.SIGNATURES["qf_stochastic_seek"][1] == [ctypes.c_void_p, ctypes.c_ulonglong]
    assert built.SIGNATURES["qf_stochastic_pattern"][1] == [ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_double,
                                                            ctypes.c_void_p, ctypes.c_void_p]
    # a null context is refused, not dereferenced
    n = ctypes.c_ulonglong()
    assert lib.qf_set_stochastic_forcing(None, 1, 2, None, 0, 0, 0.0, 0.0, 0.0, 1 << 30) == 1
    assert lib.qf_stochastic_tell(None, ctypes.byref(n)) == 1
    assert lib.qf_stochastic_seek(None, 0) == 1
    assert lib.qf_stochastic_pattern(None, 0, 0.1, None, None) == 1


def test_header_says_who_follows_and_who_refuses():
    header = open(os.path.join(REPO, "include", "quflow_hip.h")).read()
    block = header[header.index("stochastic band-limited forcing"):header.index("int qf_set_stochastic_forcing(")]
    for word in ("Philox4x32-10", "D2511F53", "CD9E8D57", "9E3779B9", "BB67AE85", "qf_isomp_forced", "qf_isomp_hooked",
                 "qf_erk_hooked", "qf_forcing", "QF_ERR_UNSUPPORTED", "band_bytes_max", "qf_slab_prefix"):
        assert word in block, word
