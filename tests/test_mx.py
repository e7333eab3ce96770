"""Block-scaled 8- and 4-bit wires with error feedback: the
host definition prophet_amd/mx.py on hand-written vectors, the compressors'
host path, and the C entry points' operand checks, which run before any device
call."""
import ctypes

import numpy as np
import pytest

from prophet_amd import mx, reducer
from prophet_amd.compression import Compression

F = np.float32
FMTS = ["fp8", "fp4"]
COMP = {"fp8": Compression.mxfp8_ef, "fp4": Compression.mxfp4_ef}
TOP = {"fp8": 0x7e, "fp4": 7}          # the code of max: 448, 6
QNAN = 0x7fc00000


def finite_codes(fmt):
    """The non-negative finite codes, ascending in value."""
    return np.arange(TOP[fmt] + 1, dtype=np.uint8)


def pinned(vals, fmt):
    """`vals` cut into blocks of 31 beside the format's max, which pins X to
    127: the scale is 1.0 and a value is its own v."""
    vals = np.asarray(vals, F)
    rows = np.zeros((-(-vals.size // 31), 31), F)
    rows.reshape(-1)[:vals.size] = vals
    top = np.full((rows.shape[0], 1), mx.value([TOP[fmt]], fmt)[0], F)
    return np.concatenate([top, rows], axis=1).reshape(-1), vals.size


def unpin(x, n):
    return x.reshape(-1, 32)[:, 1:].reshape(-1)[:n]


def edge_values(fmt):
    """Whole blocks that meet every rule of the definition (the GPU file tiles
    them): every code of both signs, every midpoint with its two float32
    neighbours, a saturating amax, subnormal and zero blocks, non-finite ones."""
    v = mx.value(finite_codes(fmt), fmt)
    mid = (v[:-1] + v[1:]) / F(2)
    near = np.concatenate([mid, np.nextafter(mid, F(0)), np.nextafter(mid, F(np.inf))])
    body = pinned(np.concatenate([v, -v, near, -near]), fmt)[0]
    sat = np.full(32, 1.0, F)
    sat[3], sat[9] = (500.0, -511.0) if fmt == "fp8" else (7.0, -7.75)
    tiny = np.full(32, 1e-40, F)
    tiny[4], tiny[5] = -0.0, -3e-45
    bad = np.full(64, 2.0, F)
    bad[7], bad[40] = np.inf, np.nan
    return np.concatenate([body, sat, tiny, np.zeros(32, F), bad, np.full(32, 3.0, F)])


@pytest.mark.parametrize("fmt", FMTS)
def test_codes_are_fixed_points_and_midpoints_go_to_even(fmt):
    codes = finite_codes(fmt)
    v = mx.value(codes, fmt)
    sign = np.uint8(1 << (mx.bits_of(fmt) - 1))
    for s, want in ((F(1), codes), (F(-1), codes | sign)):
        g, n = pinned(s * v, fmt)
        pay, r = mx.compress(g, s * np.zeros_like(g), fmt)    # -0.0 + +0.0 is +0.0
        x, q = mx.fields(pay, g.size, fmt)
        assert (x == 127).all() and np.array_equal(unpin(q, n), want)
        assert not r.any() and np.array_equal(mx.decode(pay, g.size, fmt), g)
    mid = (v[:-1] + v[1:]) / F(2)
    even = np.where(codes[:-1] % 2 == 0, codes[:-1], codes[1:])
    for vals, want in ((mid, even), (np.nextafter(mid, F(0)), codes[:-1]),
                       (np.nextafter(mid, F(np.inf)), codes[1:])):
        g, n = pinned(vals, fmt)
        assert np.array_equal(unpin(mx.quantise(g, fmt)[1], n), want)
        assert np.array_equal(unpin(mx.quantise(-g, fmt)[1], n), want | sign)


@pytest.mark.parametrize("fmt, big, x, resid", [("fp8", 500.0, 127, 52.0), ("fp8", -511.0, 127, -63.0),
                                                ("fp4", 7.0, 127, 1.0), ("fp4", -7.75, 127, -1.75),
                                                ("fp4", 2.0 ** 100 * 1.875, 225, 2.0 ** 98 * 1.5)])
def test_an_amax_past_max_saturates_into_the_residual(fmt, big, x, resid):
    g = np.full(32, 2.0 ** (x - 127), F)
    g[3] = big
    pay, r = mx.compress(g, np.zeros(32, F), fmt)
    xs, q = mx.fields(pay, 32, fmt)
    assert xs[0] == x and q[3] == TOP[fmt] | ((big < 0) << (mx.bits_of(fmt) - 1))
    assert r[3] == F(resid) and not r[np.arange(32) != 3].any()


@pytest.mark.parametrize("fmt", FMTS)
def test_small_blocks_clamp_x_to_zero_and_keep_the_sign_of_zero(fmt):
    g = np.full(32, 1e-42, F)
    g[4], g[5] = -0.0, -3e-45
    g = np.concatenate([g, np.zeros(32, F)])
    pay, r = mx.compress(g, np.copysign(F(0), g), fmt)       # -0.0 + +0.0 is +0.0
    x, q = mx.fields(pay, 64, fmt)
    sign = 1 << (mx.bits_of(fmt) - 1)
    assert not x.any()
    assert [q[0], q[4], q[5]] == [0, sign, sign] and not q[32:].any()
    # every code is 0: nothing is sent, and the residual keeps each value
    assert np.array_equal(r, g)
    assert np.array_equal(mx.decode(pay, 64, fmt).view(np.uint32) << 1, np.zeros(64, np.uint32))
    # the subnormal scale 2^-127 is used, not flushed: every code times 2^-127 is a fixed point
    g, n = pinned(mx.value(finite_codes(fmt), fmt), fmt)
    g = g * F(2.0 ** -127)
    pay, r = mx.compress(g, np.zeros_like(g), fmt)
    x, q = mx.fields(pay, g.size, fmt)
    assert not x.any() and np.array_equal(unpin(q, n), finite_codes(fmt))
    assert not r.any() and np.array_equal(mx.decode(pay, g.size, fmt), g)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("poison", [np.inf, -np.inf, np.nan])
def test_a_non_finite_block_is_nan_and_its_neighbour_is_not(fmt, poison):
    g = np.full(70, 2.0, F)                       # the ragged third block: 6 elements
    g[40] = poison
    pay, r = mx.compress(g, np.zeros(70, F), fmt)
    x, q = mx.fields(pay, 70, fmt)
    assert list(x) == [128 - mx._FORMATS[fmt][1], 255, 128 - mx._FORMATS[fmt][1]]
    assert not q[32:64].any() and q[0] != 0
    d = mx.decode(pay, 70, fmt)
    assert (d[32:64].view(np.uint32) == QNAN).all() and (r[32:64].view(np.uint32) == QNAN).all()
    assert np.array_equal(d[:32], g[:32]) and np.array_equal(d[64:], g[64:]) and not r[:32].any()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 511, 512, 513])
def test_layout(fmt, n):
    bits = mx.bits_of(fmt)
    a16 = lambda k: -(-k // 16) * 16                                    # noqa: E731
    nblk, ncode = -(-n // 32), -(-n * bits // 8)
    assert mx.payload_bytes(n, fmt) == 16 + a16(nblk) + a16(ncode)
    assert reducer.GpuReducer().lib.byteps_reduce_mx_payload_bytes(n, bits) \
        == mx.payload_bytes(n, fmt)
    g = np.arange(1, n + 1, dtype=F)
    pay, _ = mx.compress(g, np.zeros(n, F), fmt)
    assert pay.size == mx.payload_bytes(n, fmt) and mx.header(pay) == (bits, n)
    assert not pay[12:16].any()
    assert not pay[16 + nblk:16 + a16(nblk)].any() and not pay[16 + a16(nblk) + ncode:].any()
    x, q = mx.fields(pay, n, fmt)
    assert np.array_equal(q, mx.quantise(g, fmt)[1]) and (n == 0 or x.all())
    if fmt == "fp4" and n:
        raw = pay[16 + a16(nblk):16 + a16(nblk) + ncode]
        assert np.array_equal(raw & 0xf, q[0::2])                       # element 2 j: low nibble
        assert np.array_equal((raw >> 4)[:n // 2], q[1::2]) and (n % 2 == 0 or raw[-1] >> 4 == 0)


@pytest.mark.parametrize("fmt", FMTS)
def test_fold_adds_in_argument_order_then_divides(fmt):
    vals = [F(2.0 ** 24), F(1.0), F(-2.0 ** 24), F(1.0)]
    pays = [mx.compress(np.full(33, v, F), np.zeros(33, F), fmt)[0] for v in vals]
    assert (mx.fold(pays, 33, fmt) == 1.0).all()              # ((2^24 + 1) - 2^24) + 1
    assert (mx.fold(pays[::-1], 33, fmt) == 2.0).all()        # ((1 - 2^24) + 1) + 2^24
    assert (mx.fold(pays, 33, fmt, 8) == 0.125).all()
    assert np.array_equal(mx.fold(pays[:1], 33, fmt), mx.decode(pays[0], 33, fmt))
    for bad in ([], pays * 5):
        with pytest.raises(ValueError):
            mx.fold(bad, 33, fmt)
    with pytest.raises(ValueError):
        mx.fold(pays, 33, fmt, 0)


def test_error_feedback_delivers_a_small_value_beside_a_large_one():
    """Thirty-one 0.3 beside one 100.0 on the fp4 wire (X = 131, a step of 8
    at the bottom): without a residual 0.3 is sent as 0 at each of 64 steps;
    with it the small elements deliver 16.0 and hold 3.2, |r| never above 4."""
    g = np.full(32, 0.3, F)
    g[5] = 100.0
    zero = np.zeros(32, F)
    r, got, plain, worst = zero, zero.copy(), zero.copy(), 0.0
    for _ in range(64):
        p, r = mx.compress(g, r, "fp4")
        got += mx.decode(p, 32, "fp4")
        plain += mx.decode(mx.compress(g, zero, "fp4")[0], 32, "fp4")
        worst = max(worst, np.abs(np.delete(r, 5)).max())
    small = np.arange(32) != 5
    assert not plain[small].any() and (got[small] == 16.0).all() and got[5] == 6400.0
    assert np.allclose(r[small], 3.2, rtol=0, atol=2e-6) and r[5] == 0 and worst <= 4.0
    # fp8: 1e-4 lies below half the smallest step at this scale, 2^-12
    g[small] = 1e-4
    p, r = mx.compress(g, zero, "fp8")
    assert not mx.decode(p, 32, "fp8")[small].any() and (r[small] == F(1e-4)).all()


@pytest.mark.parametrize("wrap", [np.asarray, pytest.param("torch", id="torch")])
@pytest.mark.parametrize("fmt", FMTS)
def test_compressor_host_path_is_the_definition(fmt, wrap):
    if wrap == "torch":
        wrap = pytest.importorskip("torch").from_numpy
    C = COMP[fmt]
    assert C.FMT == fmt and C.ERROR_FEEDBACK and C.PACKED and not C.SERVER_ROUND
    g = np.random.default_rng(3).standard_normal(1000).astype(F)
    t, res = wrap(g.copy()), C.residual_like(wrap(g.copy()))
    pay = C.payload_like(t)
    r_ref = np.zeros(1000, F)
    for _ in range(2):
        C.compress_ef_into(pay, res, t)
        p_ref, r_ref = mx.compress(g, r_ref, fmt)
        assert np.array_equal(np.asarray(pay), p_ref) and np.array_equal(np.asarray(res), r_ref)
    out = wrap(np.empty(1000, F))
    C.fold_many_into([out], [[pay, pay]], 2)
    assert np.array_equal(np.asarray(out), mx.fold([p_ref, p_ref], 1000, fmt, 2))
    c, ctx = C.compress(t)
    assert np.array_equal(np.asarray(C.decompress(c, ctx)),
                          mx.decode(mx.compress(g, 0 * g, fmt)[0], 1000, fmt))
    i32 = wrap(np.arange(4, dtype=np.int32))
    assert C.compress(i32)[0] is i32


@pytest.mark.parametrize("fmt", FMTS)
def test_init_tensor_refuses_the_wire_over_every_front_end(fmt):
    from prophet_amd.pushpull import ServerFrontend, Worker

    class Plain:
        size = 2

    for frontend in (Plain(), ServerFrontend(server=None, size=2)):
        with pytest.raises(ValueError, match="fold_many_into"):
            Worker(0, frontend).init_tensor("g", np.zeros(8, F), 0, compression=COMP[fmt])


@pytest.mark.parametrize("fmt", FMTS)
def test_operand_checks_run_before_any_device_call(fmt):
    red = reducer.GpuReducer()
    A, B, P = 0x10000, 0x20000, 0x30000
    bad = [
        [(0, B, P, 64)], [(A, 0, P, 64)], [(A, B, 0, 64)],               # null with nelem > 0
        [(A, B, P, (1 << 31) + 1)],
        [(A + 2, B, P, 64)], [(A, B + 1, P, 64)], [(A, B, P + 8, 64)],   # alignment: 4, 4, 16
        [(A, A + 128, P, 64)], [(A, B, A + 256 - 16, 64)],               # the payload over r, g
        [(A, B, B + 16, 64)],
        [(A, B, P, 64), (A + 0x1000, B + 0x1000, P + 32, 64)],           # two segments' payloads
    ]
    for segs in bad:
        with pytest.raises(reducer.ReduceError) as e:
            red.mx_plan(segs, fmt)
        assert e.value.code == reducer.EARGS, segs
    fold_bad = [
        ([(0, [P], 64)], 1), ([(A, [0], 64)], 1), ([(A, [P + 4], 64)], 1), ([(A + 2, [P], 64)], 1),
        ([(A, [P], (1 << 31) + 1)], 1), ([(A, [P, P + 32], 64)], 2), ([(A, [A + 0x80], 64)], 1),
        ([(A, [], 64)], 0), ([(A, [P + 256 * s for s in range(17)], 64)], 17),
    ]
    for segs, nsrc in fold_bad:
        with pytest.raises(reducer.ReduceError) as e:
            red.mx_fold_plan(segs, nsrc, fmt)
        assert e.value.code == reducer.EARGS, segs
    lib, bits, h = red.lib, mx.bits_of(fmt), ctypes.c_void_p()
    desc = (reducer.MXDesc * 1)()
    for wrong in (0, 5, 16):                                            # the format
        assert lib.byteps_reduce_mx_plan_create(desc, 0, wrong, ctypes.byref(h)) == reducer.EARGS
        assert lib.byteps_reduce_mx_payload_bytes(64, wrong) == 0
    assert lib.byteps_reduce_mx_plan_compress(None, None) == reducer.EARGS
    assert lib.byteps_reduce_mx_fold_plan_launch(None, 1, None) == reducer.EARGS
    assert lib.byteps_reduce_mx_plan_destroy(None) == reducer.OK
    assert lib.byteps_reduce_mx_plan_create(None, 1, bits, ctypes.byref(h)) == reducer.EARGS
    assert lib.byteps_reduce_version() == 5
