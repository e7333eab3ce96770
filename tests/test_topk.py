"""Top-k sparsification with error feedback: the host
definition prophet_amd/topk.py, the compressor's host path, and the C entry
points' operand checks, which run before any device call."""
import ctypes

import numpy as np
import pytest

from prophet_amd import reducer, topk
from prophet_amd.compression import Compression

TK = Compression.topk_ef
F = np.float32
NAN, INF = F(np.nan), F(np.inf)


def f32(*xs):
    return np.array(xs, dtype=np.float32)


@pytest.mark.parametrize("c, k, sel", [
    (f32(1, -3, 2, -0.5), 2, [1, 2]),
    (f32(0.0, -0.0, 0.0, -0.0), 2, [0, 1]),                 # -0.0 == +0.0: the lowest indices
    (f32(1, INF, NAN, -INF, 5), 1, [2]),                    # a NaN first
    (f32(1, INF, NAN, -INF, 5), 3, [1, 2, 3]),              # then both infinities
    (f32(2, -2, 2, -2, 2), 3, [0, 1, 2]),                   # all magnitudes equal
    (f32(1, 2, 3), 3, [0, 1, 2]),                           # k == n
    (f32(4, 1, -4, 4, 9), 3, [0, 2, 4]),                    # ties cut inside the threshold
    (f32(), 0, []),                                         # n == 0
])
def test_definition_on_hand_written_vectors(c, k, sel):
    assert topk.select(c, k).tolist() == sel
    g = c * F(0.5)
    pay, rn = topk.compress(g, g, k)                        # g + g == c exactly
    assert topk.header(pay) == (k, c.size) and pay.size == 16 + 8 * k
    idx, val = topk.entries(pay)
    assert idx.tolist() == sel
    assert val.view(np.uint32).tolist() == c[sel].view(np.uint32).tolist()
    want = c.copy()
    want[sel] = 0.0
    assert rn.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    got = topk.decode(pay, c.size)
    dec = np.zeros_like(c)
    dec[sel] = c[sel]
    assert got.view(np.uint32).tolist() == dec.view(np.uint32).tolist()


@pytest.mark.parametrize("k", [1, 3])
def test_payload_layout(k):
    g = f32(0.5, -7, 0, 3, -2)
    pay, _ = topk.compress(g, np.zeros(5, F), k)
    sel = [1] if k == 1 else [1, 3, 4]
    want = np.array([k, 5, 0, 0] + sel, "<u4").tobytes() + g[sel].astype("<f4").tobytes()
    assert pay.tobytes() == want and topk.payload_bytes(k) == len(want)
    assert topk.k_of(pay) == k
    assert [topk.k_for(n, 0.01) for n in (0, 1, 100, 101, 5)] == [0, 1, 1, 2, 1]
    assert topk.k_for(7, 2.0) == 7


def test_fold_order_with_overlapping_indices():
    big, n = F(2.0 ** 24), 8

    def payload(idx, val):
        return np.concatenate([np.array([len(idx), n, 0, 0] + idx, "<u4").view(np.uint8),
                               np.array(val, "<f4").view(np.uint8)])
    a, b, c = payload([1, 5], [big, 1]), payload([1, 6], [1, 2]), payload([1, 5], [-big, 1])
    assert topk.fold([a, b, c], n).tolist() == [0, 0, 0, 0, 0, 2, 2, 0]     # (2^24 + 1) - 2^24
    assert topk.fold([a, c, b], n).tolist() == [0, 1, 0, 0, 0, 2, 2, 0]
    assert topk.fold([a, c, b], n, 8).tolist() == [0, 0.125, 0, 0, 0, 0.25, 0.25, 0]
    assert np.signbit(topk.decode(payload([0, 1], [-0.0, 1]), n)[0])       # out[idx] = val
    assert not np.signbit(topk.fold([payload([0, 1], [-0.0, 1])], n)[0])   # +0.0 + -0.0
    with pytest.raises(ValueError):
        topk.fold([a] * 17, n)
    with pytest.raises(ValueError):
        topk.fold([a], n, 0)


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_compressor_host_path(kind):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    g = rng.standard_normal(1000).astype(F)
    wrap = (lambda a: a) if kind == "numpy" else torch.from_numpy
    assert TK.PACKED and TK.ERROR_FEEDBACK
    assert TK.compresses(wrap(g)) and not TK.compresses(wrap(g.astype(np.float64)))
    t = wrap(g.copy())
    pay, res = TK.payload_like(t, 0.05), TK.residual_like(t)
    assert topk.k_of(pay) == 50
    r_ref = np.zeros(1000, F)
    for _ in range(2):
        TK.compress_ef_into(pay, res, t)
        p_ref, r_ref = topk.compress(g, r_ref, 50)
        assert np.array_equal(np.asarray(pay), p_ref) and np.array_equal(np.asarray(res), r_ref)
    out = wrap(np.empty(1000, F))
    TK.fold_many_into([out], [[pay, pay]], 2)
    assert np.array_equal(np.asarray(out), topk.fold([p_ref, p_ref], 1000, 2))
    TK.decompress_into(out, pay)
    assert np.array_equal(np.asarray(out), topk.fold([p_ref], 1000))
    c, ctx = TK.compress(t, 0.05)
    assert np.array_equal(np.asarray(TK.decompress(c, ctx)),
                          topk.fold([topk.compress(g, 0 * g, 50)[0]], 1000))


def test_error_feedback_delivers_a_small_value_beside_large_ones():
    """One gradient — 1e-3 beside 63 values of 1.0 — then zeros, at k = 1: the
    residual hands the 64 values over one a step, the small one last, exactly;
    top-1 without a residual sends one large value and never the small one.
    (Under a gradient repeated every step the 63 large residuals grow by 63 a
    step and shrink by one entry: no top-1 ever reaches the small value.)"""
    g = np.full(64, 1.0, F)
    g[17] = 1e-3
    zero = np.zeros(64, F)
    r, got, plain = zero, zero.copy(), zero.copy()
    for t in range(64):
        gt = g if t == 0 else zero
        p, r = topk.compress(gt, r, 1)
        got += topk.decode(p, 64)
        plain += topk.decode(topk.compress(gt, zero, 1)[0], 64)
        assert (got[17] != 0) == (t == 63)
    assert np.array_equal(got, g) and not r.any()
    assert plain[17] == 0 and plain.sum() == 1.0


def test_init_tensor_refuses_topk_over_every_front_end():
    from prophet_amd.pushpull import ServerFrontend, Worker

    class Plain:
        size = 2

    for frontend in (Plain(), ServerFrontend(server=None, size=2)):
        with pytest.raises(ValueError, match="fold_many_into"):
            Worker(0, frontend).init_tensor("g", np.zeros(8, F), 0, compression=TK)


def test_operand_checks_run_before_any_device_call():
    red = reducer.GpuReducer()
    A, B, P = 0x10000, 0x20000, 0x30000
    bad = [
        [(0, B, P, 64, 4)], [(A, 0, P, 64, 4)], [(A, B, 0, 64, 4)],       # null with nelem > 0
        [(A, B, P, 64, 0)], [(A, B, P, 64, 65)], [(0, 0, P, 0, 1)],       # k outside 1..nelem
        [(A, B, P, (1 << 31) + 1, 4)],
        [(A, B, P + 8, 64, 4)],                                          # payload alignment
        [(A, A + 128, P, 64, 4)], [(A, B, A + 256 - 16, 64, 4)],           # overlaps
        [(A, B, P, 64, 4), (A + 0x1000, B + 0x1000, P + 32, 64, 4)],       # two segments' payloads
    ]
    for segs in bad:
        with pytest.raises(reducer.ReduceError) as e:
            red.topk_plan(segs)
        assert e.value.code == reducer.EARGS, segs
    fold_bad = [
        ([(0, [P], 64, 4)], 1), ([(A, [0], 64, 4)], 1), ([(A, [P + 4], 64, 4)], 1),
        ([(A, [P], 64, 0)], 1), ([(A, [P], 64, 65)], 1), ([(A, [P], (1 << 31) + 1, 4)], 1),
        ([(A, [P, P], 64, 4)], 2), ([(A, [P, P + 32], 64, 4)], 2), ([(A, [A + 0x80], 64, 4)], 1),
        ([(A, [], 64, 4)], 0), ([(A, [P + 64 * s for s in range(17)], 64, 4)], 17),
    ]
    for segs, nsrc in fold_bad:
        with pytest.raises(reducer.ReduceError) as e:
            red.topk_fold_plan(segs, nsrc)
        assert e.value.code == reducer.EARGS, segs
    lib = red.lib
    assert lib.byteps_reduce_topk_payload_bytes(3) == 40
    assert lib.byteps_reduce_topk_plan_compress(None, None) == reducer.EARGS
    assert lib.byteps_reduce_topk_fold_plan_launch(None, 1, None) == reducer.EARGS
    assert lib.byteps_reduce_topk_plan_destroy(None) == reducer.OK
    assert lib.byteps_reduce_topk_plan_create(None, 1, ctypes.byref(ctypes.c_void_p())) \
        == reducer.EARGS
    assert lib.byteps_reduce_version() == 5
