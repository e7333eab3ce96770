"""1-bit sign compression with error feedback on the host:
prophet_amd/onebit.py, the definition, on hand-written vectors; the host path
of Compression.onebit_ef; what error feedback delivers; and the operand checks
of byteps_reduce_onebit_*, which run before any HIP call."""
import ctypes
import math

import numpy as np
import pytest

from prophet_amd import onebit, reducer
from prophet_amd.compression import Compression

OB = Compression.onebit_ef


def f32(*xs):
    return np.array(xs, dtype=np.float32)


def test_definition_on_hand_written_vectors():
    # sum |c| = 4, n = 4: scale 1; -0.0 and +0.0 are not negative
    p, r = onebit.compress(f32(-2.5, 1.0, -0.0, 0.0), f32(-0.5, 0.0, 0.0, 0.0))
    assert onebit.header(p) == (np.float32(1.0), 4)
    assert p.size == 24 and p[16] == 0b0001 and not p[17:].any()
    assert r.tobytes() == f32(-2.0, 0.0, -1.0, -1.0).tobytes()
    assert onebit.decode(p, 4).tobytes() == f32(-1.0, 1.0, 1.0, 1.0).tobytes()
    # a NaN is not negative; it poisons the scale, and with it every residual
    p, r = onebit.compress(f32(np.nan, -1.0), f32(0.0, 0.0))
    assert np.isnan(onebit.header(p)[0]) and list(onebit.bits(p, 2)) == [False, True]
    assert np.isnan(r).all()
    p, r = onebit.compress(f32(), f32())
    assert p.tobytes() == bytes(16)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_payload_layout(n):
    assert onebit.payload_bytes(n) == 16 + 8 * math.ceil(n / 64)
    assert reducer.load_library().byteps_reduce_onebit_payload_bytes(n) == onebit.payload_bytes(n)
    g = -np.ones(n, dtype=np.float32)             # every bit set
    p, r = onebit.compress(g, np.zeros(n, dtype=np.float32))
    words = p[16:].view("<u8")
    assert onebit.header(p) == (np.float32(1.0), n) and not p[12:16].any()
    want = [(1 << 64) - 1] * (n // 64) + ([(1 << (n % 64)) - 1] if n % 64 else [])
    assert list(map(int, words)) == want          # the bits past n are 0
    assert not r.any()


def test_fold_is_a_left_fold_then_a_divide():
    big, n = np.float32(2.0 ** 24), 3
    ps = [onebit.compress(np.full(n, v, np.float32), np.zeros(n, np.float32))[0]
          for v in (big, 1.0, -big)]
    assert list(onebit.fold(ps, n)) == [0.0] * n              # (2^24 + 1) - 2^24
    assert list(onebit.fold([ps[0], ps[2], ps[1]], n, 8)) == [0.125] * n
    assert onebit.fold(ps[2:], n).tobytes() == np.full(n, -big, np.float32).tobytes()


def test_exact_inputs_have_an_order_independent_sum():
    """Kind (a) of the GPU tests: multiples of 2^-10 whose total stays far
    below 2^53 units, so every order of the f64 sum gives the same bits."""
    rng = np.random.default_rng(5)
    a = np.abs(rng.integers(-4096, 4097, 20_000).astype(np.float32) * np.float32(2.0 ** -10))
    a = a.astype(np.float64)
    pair = a.copy()
    while pair.size > 1:
        if pair.size % 2:
            pair = np.append(pair, 0.0)
        pair = pair[0::2] + pair[1::2]
    rev = 0.0
    for x in a[::-1]:
        rev += x
    assert math.fsum(a) == rev == pair[0] == float(a.sum())


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_compressor_host_path(kind):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    gs = [rng.standard_normal(n).astype(np.float32) for n in (1, 65, 300)]
    rs = [rng.standard_normal(g.size).astype(np.float32) * np.float32(0.1) for g in gs]
    want = [onebit.compress(g, r) for g, r in zip(gs, rs)]
    wrap = (lambda x: torch.from_numpy(x.copy())) if kind == "torch" else (lambda x: x.copy())
    tens, res = [wrap(g) for g in gs], [wrap(r) for r in rs]
    pay = [OB.payload_like(t) for t in tens]
    assert OB.compresses(tens[0]) and not OB.compresses(wrap(gs[0].astype(np.float64)))
    OB.compress_many_ef_into(pay, res, tens)
    for p, r, (wp, wr) in zip(pay, res, want):
        assert np.asarray(p).tobytes() == wp.tobytes() and np.asarray(r).tobytes() == wr.tobytes()
    outs = [wrap(np.empty_like(g)) for g in gs]
    OB.fold_many_into(outs, [[p, p, p] for p in pay], divisor=2)
    for o, (wp, _), g in zip(outs, want, gs):
        assert np.asarray(o).tobytes() == onebit.fold([wp] * 3, g.size, 2).tobytes()
    one = OB.decompress_into(wrap(np.empty_like(gs[1])), pay[1])
    assert np.asarray(one).tobytes() == onebit.decode(want[1][0], 65).tobytes()


def test_error_feedback_delivers_a_small_value_beside_large_ones():
    """One step decodes 1e-3 as +scale, about 0.98.  Over T steps the decodes
    add up to T g - r_T but for the roundings of 2 f32 operations a step on
    values below 4 (2^-22 each at most), and r stays within two scales."""
    g = np.full(64, 1.0, dtype=np.float32)
    g[-1] = 1e-3
    r = np.zeros(64, dtype=np.float32)
    T, total = 20_000, 0.0
    for t in range(T):
        p, r = onebit.compress(g, r)
        d = float(onebit.decode(p, 64)[-1])
        if t == 0:
            assert abs(d - 1e-3) > 0.9
        total += d
    assert abs(r[-1]) <= 2.0
    assert abs(total - (T * float(g[-1]) - float(r[-1]))) <= T * 2.0 ** -21
    assert abs(total / T - 1e-3) <= 2.0 / T + 2.0 ** -21


def test_init_tensor_refuses_the_packed_wire():
    from prophet_amd.pushpull import Worker

    class Frontend:
        size = 2

    w = Worker(0, Frontend())
    with pytest.raises(ValueError, match="fold_many_into"):
        w.init_tensor("g", np.zeros(8, np.float32), 0, compression=OB)


def test_operand_checks_run_before_any_device_call():
    red = reducer.GpuReducer()
    A, B, P = 0x10000, 0x20000, 0x30000
    bad = [
        [(0, B, P, 64)], [(A, 0, P, 64)], [(A, B, 0, 64)],          # null with nelem > 0
        [(A, B, P + 8, 64)],                                       # payload not 16-byte aligned
        [(A, A + 128, P, 64)], [(A, B, A + 256 - 16, 64)],           # overlaps
        [(A, B, P, 64), (A + 0x1000, B + 0x1000, P + 16, 64)],       # two segments' payloads
        [(A, B, P, (1 << 37) + 1)],
    ]
    for segs in bad:
        with pytest.raises(reducer.ReduceError) as e:
            red.onebit_plan(segs)
        assert e.value.code == reducer.EARGS, segs
    fold_bad = [
        ([(0, [P], 64)], 1), ([(A, [0], 64)], 1), ([(A, [P + 4], 64)], 1),
        ([(A, [P, P], 64)], 2), ([(A, [A + 0x80], 64)], 1),
        ([(A, [], 64)], 0), ([(A, [P + 32 * k for k in range(17)], 64)], 17),
    ]
    for segs, nsrc in fold_bad:
        with pytest.raises(reducer.ReduceError) as e:
            red.onebit_fold_plan(segs, nsrc)
        assert e.value.code == reducer.EARGS, segs
    lib = red.lib
    assert lib.byteps_reduce_onebit_plan_compress(None, None) == reducer.EARGS
    assert lib.byteps_reduce_onebit_fold_plan_launch(None, 1, None) == reducer.EARGS
    assert lib.byteps_reduce_onebit_plan_destroy(None) == reducer.OK
    assert lib.byteps_reduce_onebit_plan_create(None, 1, ctypes.byref(ctypes.c_void_p())) \
        == reducer.EARGS
