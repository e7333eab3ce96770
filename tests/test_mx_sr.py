"""The stateless block-scaled wires: prophet_amd/mx_sr.py,
the definition, on the CPU — unbiased rounding, the scale that never clamps,
the rotation and its fold, non-finite blocks, the layout, the compressors' host
path and the C entry points' operand checks."""
import ctypes

import numpy as np
import pytest

from prophet_amd import mx, mx_sr, reducer, sr
from prophet_amd.compression import Compression

F = np.float32
CASES = [(fmt, rot) for fmt in ("fp8", "fp4") for rot in (False, True)]
COMP = {("fp8", False): Compression.mxfp8_sr, ("fp4", False): Compression.mxfp4_sr,
        ("fp8", True): Compression.mxfp8_rht_sr, ("fp4", True): Compression.mxfp4_rht_sr}
MANT = {"fp8": 0x600000, "fp4": 0x400000}
case = pytest.mark.parametrize("fmt, rot", CASES)
fmts = pytest.mark.parametrize("fmt", ["fp8", "fp4"])


def f32(bits):
    return np.asarray(bits, np.uint32).view(F)


def edge_blocks(fmt):
    """Blocks of 32 the GPU file tiles: on-grid codes, values between them, a
    top mantissa at MANT and one ulp past it, a subnormal block, +-0, and blocks
    with an inf and a NaN."""
    vmax = mx._fmt(fmt)[2]
    grid = mx.value(np.arange(32) % (1 << (mx.bits_of(fmt) - 1)), fmt)
    grid = np.where(np.isnan(grid), F(vmax), grid).astype(F)
    between = (np.linspace(-vmax, vmax, 32) * 0.77).astype(F)
    at = np.full(32, 0.3, F)
    at[3] = f32(0x42000000 | MANT[fmt])
    past = at.copy()
    past[3] = f32((0x42000000 | MANT[fmt]) + 1)
    tiny = (np.linspace(-1, 1, 32) * 2.0 ** -140).astype(F)
    zeros = np.where(np.arange(32) % 2, F(-0.0), F(0.0))
    inf, nan = between.copy(), between.copy()
    inf[9], nan[31] = np.inf, np.nan
    return np.concatenate([grid, between, at, past, tiny, zeros, inf, between, nan])


@fmts
def test_rounding_is_unbiased_over_every_r16(fmt):
    _, _, vmax, mbits, bias = mx._fmt(fmt)
    r16 = np.arange(65536)
    for v in (vmax * 0.99, 1.3, -2.7, 1.0001, 2.0 ** (1 - bias) * 0.37, 2.0 ** (-bias - mbits)):
        d = mx.value(mx_sr.sr_encode(np.full(65536, v, F), r16, fmt), fmt).astype(np.float64)
        step = np.ptp(np.unique(d))               # f floors the fraction: never above |v|
        assert np.all(np.signbit(d) == (v < 0))
        assert step > 0 and 0 <= abs(float(F(v))) - np.abs(d).mean() <= step * 2.0 ** -16, v
    grid = mx.value(np.arange(1 << mx.bits_of(fmt)), fmt)
    for v in grid[np.isfinite(grid)]:
        q = mx_sr.sr_encode(np.full(65536, v, F), r16, fmt)
        assert np.array_equal(mx.value(q, fmt).view(np.uint32),
                              np.full(65536, v, F).view(np.uint32)), v


@fmts
def test_the_scale_never_clamps_and_the_codes_bracket(fmt):
    emax, vmax = mx._fmt(fmt)[1:3]
    rng = np.random.default_rng(0)
    c = (rng.standard_normal((500, 32)) * np.exp2(rng.integers(-40, 41, (500, 1)))).astype(F)
    x = mx_sr.scales(c, fmt)
    v = c * mx._pow2(254 - x.astype(np.int64))[:, None]
    assert np.abs(v).max() <= vmax
    lo = mx.value(mx_sr.quantise(c, np.zeros(c.size), fmt)[1], fmt).reshape(c.shape)
    hi = mx.value(mx_sr.quantise(c, np.full(c.size, 0xffff), fmt)[1], fmt).reshape(c.shape)
    assert np.all(np.abs(lo) <= np.abs(v)) and np.all(np.abs(v) <= np.abs(hi))
    assert np.all(np.signbit(lo) == np.signbit(v))
    top = np.zeros(32, F)
    top[5] = -f32(0x42000000 | MANT[fmt])            # 2^5 times the largest unbumped mantissa
    assert mx_sr.scales(top, fmt)[0] == 132 - emax
    top[5] = -f32((0x42000000 | MANT[fmt]) + 1)
    assert mx_sr.scales(top, fmt)[0] == 133 - emax


@fmts
def test_rotation_round_trips_and_folds_to_the_mean(fmt):
    one = np.zeros(96, F)
    one[[7, 40]] = [4.0, -0.5]
    p = mx_sr.compress(one, fmt, 3, 9, True, 77)
    assert mx_sr.rotated(p) and not mx_sr.rotated(mx_sr.compress(one, fmt, 3, 9))
    assert np.array_equal(mx_sr.fold([p], 96, fmt, 1, True, 77, 9), one)
    a, b = np.zeros(64, F), np.zeros(64, F)
    a[3], b[3], b[50] = 2.0, 4.0, -1.0
    pa, pb = (mx_sr.compress(g, fmt, k, 5, True, 1234) for g, k in ((a, 1), (b, 2)))
    assert np.array_equal(mx_sr.fold([pa, pb], 64, fmt, 2, True, 1234, 5), (a + b) / 2)
    assert not np.array_equal(mx_sr.fold([pa, pb], 64, fmt, 2, True, 1235, 5), (a + b) / 2)
    # a last block of fewer than 32 elements travels unrotated
    g = np.arange(40, dtype=F)
    pr, pu = mx_sr.compress(g, fmt, 3, 9, True, 77), mx_sr.compress(g, fmt, 3, 9)
    assert np.array_equal(mx.fields(pr, 40, fmt)[1][32:], mx.fields(pu, 40, fmt)[1][32:])
    assert mx.fields(pr, 40, fmt)[0][1] == mx.fields(pu, 40, fmt)[0][1]


@case
@pytest.mark.parametrize("poison", [np.inf, np.nan])
def test_a_non_finite_block_is_x255_and_folds_to_nan(fmt, rot, poison):
    g = np.linspace(-3, 3, 70).astype(F)
    g[40] = poison
    p, clean = (mx_sr.compress(x, fmt, 1, 2, rot, 8) for x in (g, np.ones(70, F)))
    x, q = mx.fields(p, 70, fmt)
    assert list(x == 255) == [False, True, False] and not q[32:64].any()
    out = mx_sr.fold([clean, p], 70, fmt, 2, rot, 8, 2).view(np.uint32)
    assert np.all(out[32:64] == 0x7fc00000)
    assert np.isfinite(out[:32].view(F)).all() and np.isfinite(out[64:].view(F)).all()


@case
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 513])
def test_layout(fmt, rot, n):
    g = np.random.default_rng(n).standard_normal(n).astype(F)
    p = mx_sr.compress(g, fmt, 11, 4, rot, 6)
    blocks, codes = -(-n // 32), (n * mx.bits_of(fmt) + 7) // 8
    assert p.size == mx.payload_bytes(n, fmt) == 16 + (blocks + 15) // 16 * 16 + (codes + 15) // 16 * 16
    assert list(p[:16].view("<u4")) == [mx.bits_of(fmt), n, 0, int(rot)]
    at = 16 + (blocks + 15) // 16 * 16
    assert not p[16 + blocks:at].any() and not p[at + codes:].any()
    assert mx.header(p) == (mx.bits_of(fmt), n)


@case
@pytest.mark.parametrize("wrap", [np.asarray, pytest.param("torch", id="torch")])
def test_compressor_host_path_is_the_definition(fmt, rot, wrap):
    if wrap == "torch":
        wrap = pytest.importorskip("torch").from_numpy
    C = COMP[(fmt, rot)]
    assert (C.STOCHASTIC, C.PACKED, C.ERROR_FEEDBACK, C.SERVER_ROUND, C.FMT, C.ROTATE) == \
        (True, True, False, False, fmt, rot)
    gs = [np.random.default_rng(n).standard_normal(n).astype(F) for n in (77, 256)]
    keys, rks = [5, 6], [mx_sr.rotation_key(k, 42) for k in (0, 1)]
    assert rks[0] == int(sr.philox2x32(0, 0, 42)[1]) and rks[0] != rks[1]
    T = [wrap(g.copy()) for g in gs]
    P = [C.payload_like(t) for t in T]
    C.compress_many_sr_into(P, T, keys, 3, rks)
    want = [mx_sr.compress(g, fmt, k, 3, rot, rk) for g, k, rk in zip(gs, keys, rks)]
    for p, w in zip(P, want):
        assert np.array_equal(np.asarray(p), w)
    outs = [wrap(np.empty(g.size, F)) for g in gs]
    C.fold_many_into(outs, [[p, p] for p in P], 2, rot_keys=rks, step=3)
    for o, w, g, rk in zip(outs, want, gs, rks):
        assert np.array_equal(np.asarray(o), mx_sr.fold([w, w], g.size, fmt, 2, rot, rk, 3))
    pay, ctx = C.compress(T[0], key=5, step=3, rot_key=rks[0])
    assert np.array_equal(np.asarray(pay), want[0])
    assert np.array_equal(np.asarray(C.decompress(pay, ctx)),
                          mx_sr.fold([want[0]], 77, fmt, 1, rot, rks[0], 3))
    i32 = wrap(np.arange(4, dtype=np.int32))
    assert C.compress(i32)[0] is i32


@case
def test_init_tensor_refuses_the_wire_over_every_front_end(fmt, rot):
    from prophet_amd.pushpull import ServerFrontend, Worker

    class Plain:
        size = 2

    for frontend in (Plain(), ServerFrontend(server=None, size=2)):
        with pytest.raises(ValueError, match="fold_many_into"):
            Worker(0, frontend).init_tensor("g", np.zeros(8, F), 0, compression=COMP[(fmt, rot)])


@fmts
def test_operand_checks_run_before_any_device_call(fmt):
    red = reducer.GpuReducer()
    A, P = 0x10000, 0x30000
    bad = [
        [(0, P, 64, 1, 2)], [(A, 0, 64, 1, 2)],                          # null with nelem > 0
        [(A, P, (1 << 31) + 1, 1, 2)],
        [(A + 2, P, 64, 1, 2)], [(A, P + 8, 64, 1, 2)],                  # alignment: 4, 16
        [(A, A + 256 - 16, 64, 1, 2)],                                   # the payload over g
        [(A, P, 64, 1, 2), (A + 0x1000, P + 32, 64, 1, 2)],              # two segments' payloads
    ]
    for segs in bad:
        for rotate in (False, True):
            with pytest.raises(reducer.ReduceError) as e:
                red.mx_sr_plan(segs, fmt, rotate)
            assert e.value.code == reducer.EARGS, segs
    fold_bad = [
        ([(0, [P], 64, 7)], 1), ([(A, [0], 64, 7)], 1), ([(A, [P + 4], 64, 7)], 1),
        ([(A + 2, [P], 64, 7)], 1), ([(A, [P], (1 << 31) + 1, 7)], 1),
        ([(A, [P, P + 32], 64, 7)], 2), ([(A, [A + 0x80], 64, 7)], 1), ([(A, [], 64, 7)], 0),
        ([(A, [P + 256 * s for s in range(17)], 64, 7)], 17),
    ]
    for segs, nsrc in fold_bad:
        with pytest.raises(reducer.ReduceError) as e:
            red.mx_rht_fold_plan(segs, nsrc, fmt)
        assert e.value.code == reducer.EARGS, segs
    lib, bits, h = red.lib, mx.bits_of(fmt), ctypes.c_void_p()
    desc, fdesc = (reducer.MXSRDesc * 1)(), (reducer.MXRHTFoldDesc * 1)()
    for wrong in (0, 5, 16):                                            # the format
        assert lib.byteps_reduce_mx_sr_plan_create(desc, 0, wrong, 0, ctypes.byref(h)) == reducer.EARGS
        assert lib.byteps_reduce_mx_rht_fold_plan_create(fdesc, 0, 1, wrong,
                                                         ctypes.byref(h)) == reducer.EARGS
    for rotate in (-1, 2):
        assert lib.byteps_reduce_mx_sr_plan_create(desc, 0, bits, rotate,
                                                   ctypes.byref(h)) == reducer.EARGS
    assert lib.byteps_reduce_mx_sr_plan_compress(None, 0, None) == reducer.EARGS
    assert lib.byteps_reduce_mx_rht_fold_plan_launch(None, 1, 0, None) == reducer.EARGS
    assert lib.byteps_reduce_mx_sr_plan_create(None, 1, bits, 0, ctypes.byref(h)) == reducer.EARGS
    assert lib.byteps_reduce_version() == 5
