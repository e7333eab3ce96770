"""PowerSGD low-rank compression: the host definition
prophet_amd/powersgd.py on hand-written and low-rank inputs, the compressor's
host path, and the C entry points' operand checks, which run before any device
call."""
import ctypes

import numpy as np
import pytest

from prophet_amd import powersgd, reducer
from prophet_amd.compression import Compression

F, D = np.float32, np.float64
C = Compression.powersgd_ef
U = 2.0 ** -24


def low_rank(rng, n, m, k):
    """Exactly of rank k in float32: small integer factors."""
    return (rng.integers(-8, 9, (n, k)) @ rng.integers(-8, 9, (k, m))).astype(F)


def step(g, R, Q, dtype):
    """One single-worker iteration; returns (out, Qn)."""
    P = powersgd.project_p(g, R, Q, dtype=dtype)
    powersgd.orthogonalize(P, dtype=dtype)
    Qn = powersgd.project_q(R, P, dtype=dtype)
    return powersgd.finish(np.empty(R.shape, dtype), R, P, Qn, dtype=dtype), Qn


def test_the_definition_on_a_rank_one_matrix_by_hand():
    u, v = np.array([1, 2, 2], F), np.array([1, 0, 2, 2], F)
    g, R = np.outer(u, v), np.zeros((3, 4), F)
    P = powersgd.project_p(g, R, np.array([[1], [0], [0], [0]], F))
    assert np.array_equal(R, g) and np.array_equal(P, u[:, None])
    powersgd.orthogonalize(P)
    assert np.array_equal(P, np.array([[1 / 3], [2 / 3], [2 / 3]], F))     # |u| = 3
    Qn = powersgd.project_q(R, P)
    assert np.allclose(Qn[:, 0], 3 * v, rtol=2 * U, atol=0)
    out = powersgd.finish(np.empty((3, 4), F), R, P, np.array(3 * v[:, None], F))
    assert np.array_equal(out, g) and not R.any()                          # f32(1/3) * 3 is 1.0
    # a zero and a non-finite column are dropped; a non-finite element leaves no residual
    Z = np.array([[1, 0, np.inf], [1, 0, 1]], F)
    assert np.array_equal(powersgd.orthogonalize(Z)[:, 1:], np.zeros((2, 2), F))
    R = np.array([[np.inf, 5.0]], F)
    powersgd.finish(np.empty((1, 2), F), R, np.ones((1, 1), F), np.array([[1], [2]], F))
    assert np.array_equal(R, np.array([[0.0, 3.0]], F))


def test_compresses_is_the_shape_rule():
    z = lambda *s: np.zeros(s, F)                                          # noqa: E731
    assert powersgd.shape_of(z(512, 512, 3, 3)) == (512, 4608)
    assert powersgd.compresses(z(512, 512, 3, 3), 4) and C.compresses(z(64, 64, 3, 3), 16)
    assert not powersgd.compresses(z(4608), 1)                             # a vector
    assert powersgd.compresses(z(3, 4), 1) and not powersgd.compresses(z(2, 2), 1)   # 7 < 12, 4 = 4
    assert not powersgd.compresses(np.zeros((64, 64), D), 4)
    assert not powersgd.compresses(np.zeros((64, 64), np.int32), 4)
    assert C.state_like(z(2, 2), 1, 0) is None
    for r in (0, 17):
        with pytest.raises(ValueError):
            powersgd.compresses(z(64, 64), r)
    st = C.state_like(z(6, 5, 2), 2, 7)
    assert (st.n, st.m, st.P.shape, st.Qn.shape) == (6, 10, (6, 2), (10, 2)) and not st.R.any()
    assert np.array_equal(st.Q, powersgd.init_q(10, 2, 7)) and st.Q.dtype == F


@pytest.mark.parametrize("wrap", [np.asarray, pytest.param("torch", id="torch")])
def test_compressor_host_path_is_the_definition(wrap):
    if wrap == "torch":
        wrap = pytest.importorskip("torch").from_numpy
    assert C.ERROR_FEEDBACK
    rng = np.random.default_rng(3)
    g = rng.standard_normal((12, 5, 4)).astype(F)
    R, Q = np.zeros((12, 20), F), powersgd.init_q(20, 3, 11)
    t, st = wrap(g.copy()), C.state_like(wrap(g.copy()), 3, 11)
    for _ in range(2):
        t[:] = wrap(g.copy())
        C.project_p_many([t], [st])
        C.orthogonalize_many([t], [st])
        C.project_q_many([t], [st])
        C.finish_many([t], [st])
        out, Q = step(g, R, Q, F)
        for got, want in ((t, out), (st.R, R), (st.Q, Q)):
            assert np.array_equal(np.asarray(got).reshape(want.shape), want)
    with pytest.raises(ValueError):
        C.project_p_many([wrap(np.zeros(8, F))], [st])
    with pytest.raises(ValueError, match="contiguous"):     # a reshaped copy would lose the writes
        C.project_p_many([wrap(np.zeros((12, 5, 8), F))[:, :, ::2]], [st])


@pytest.mark.parametrize("n, m, r", [(40, 50, 3), (7, 300, 1)])
def test_an_exactly_rank_r_matrix_is_delivered_whole(n, m, r):
    """The float64 evaluation returns g and leaves nothing; the float32 one is
    held to 16 times its own distance from that, the end-to-end tolerance of
    the device's round, itself under a dot product's bound over n + m terms."""
    g = low_rank(np.random.default_rng(n), n, m, r)
    Q = powersgd.init_q(m, r, 5)
    R32, R64 = np.zeros((n, m), F), np.zeros((n, m), D)
    out32, out64 = step(g, R32, Q, F)[0], step(g, R64, Q, D)[0]
    err = np.abs(out32 - out64).max()
    assert np.abs(out64 - g).max() < 1e-12 * np.abs(g).max() and np.abs(R64).max() < 1e-12
    assert 0 < err <= 64 * r * (n + m) * U * np.abs(g).max()
    assert np.abs(R32).max() <= 16 * err


def test_error_feedback_delivers_what_the_rank_dropped():
    """A rank-2 gradient at r = 1, then zero gradients: every step takes one
    direction out of the residual, so the outs add up to g after two."""
    g = low_rank(np.random.default_rng(9), 30, 20, 2)
    R, Q, total = np.zeros((30, 20), F), powersgd.init_q(20, 1, 1), np.zeros((30, 20), D)
    left = []
    for it in range(3):
        out, Q = step(g if it == 0 else np.zeros_like(g), R, Q, F)
        total += out
        left.append(np.linalg.norm(total - g) / np.linalg.norm(g))
    assert left[0] > 0.05 and left[1] < 1e-5 and left[2] < 1e-5
    assert np.linalg.norm(R) < 1e-5 * np.linalg.norm(g)


def test_init_tensor_refuses_the_compressor():
    from prophet_amd.pushpull import ServerFrontend, Worker
    with pytest.raises(ValueError):
        Worker(0, ServerFrontend(server=None, size=2)).init_tensor(
            "g", np.zeros((8, 8), F), 0, compression=C)


def test_operand_checks_run_before_any_device_call():
    red = reducer.GpuReducer()
    G, R, P, Q, N, O = (0x100000 * k for k in range(1, 7))
    ok = (G, R, P, Q, N, O, 64, 64)

    def seg(**kw):
        s = dict(zip("grpqnoNM", ok))
        s.update(kw)
        return [tuple(s[k] for k in "grpqnoNM")]
    bad = [seg(**{k: 0}) for k in "grpqno"]                                # null pointers
    bad += [seg(**{k: s + 8}) for k, s in zip("grpqno", ok)]               # 16-byte alignment
    bad += [seg(r=G + 64), seg(o=R), seg(p=G + 4096), seg(q=P + 512), seg(n=Q),     # overlaps
            seg(o=G + 16), seg(N=0), seg(M=0), seg(N=(1 << 24) + 1), seg(N=1 << 20, M=1 << 14),
            seg() + seg(g=0x900000, r=0xa00000, p=0xb00000, q=0xc00000, n=0xd00000)]  # out, twice
    for segs in bad:
        with pytest.raises(reducer.ReduceError) as e:
            red.powersgd_plan(segs, 4)
        assert e.value.code == reducer.EARGS, segs
    for rank in (0, 17):
        with pytest.raises(reducer.ReduceError) as e:
            red.powersgd_plan(seg(), rank)
        assert e.value.code == reducer.EARGS
    lib, h = red.lib, ctypes.c_void_p()
    assert lib.byteps_reduce_powersgd_plan_create(None, 1, 4, ctypes.byref(h)) == reducer.EARGS
    for phase in ("project_p", "orthogonalize", "project_q", "finish"):
        assert getattr(lib, "byteps_reduce_powersgd_plan_" + phase)(None, None) == reducer.EARGS
    assert lib.byteps_reduce_powersgd_plan_destroy(None) == reducer.OK
    assert lib.byteps_reduce_powersgd_scratch_bytes(64, 576, 4) == 9 * 64 * 4 * 4
    assert lib.byteps_reduce_powersgd_scratch_bytes(64, 576, 17) == 0
    assert lib.byteps_reduce_version() == 5
