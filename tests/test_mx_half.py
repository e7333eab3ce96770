"""The block-scaled wires over float16 and bfloat16 tensors
on the CPU: the definition on a half input is the definition on its exact
upcast, a fold converts its float32 result once, the compressors' host path,
and the typed plan creates' operand checks.  Byte for byte throughout."""
import ctypes

import numpy as np
import pytest

from prophet_amd import mx, mx_sr, reducer
from prophet_amd.compression import Compression
from prophet_amd.dtypes import DType

torch = pytest.importorskip("torch")

F = np.float32
WIRES = [(fmt, kind) for fmt in ("fp8", "fp4") for kind in ("ef", "sr", "rht")]
COMP = {(fmt, kind): getattr(Compression, f"mx{fmt}_{'rht_sr' if kind == 'rht' else kind}")
        for fmt, kind in WIRES}
wires = pytest.mark.parametrize("fmt, kind", WIRES)
dtypes = pytest.mark.parametrize("dt", ["float16", "bfloat16"])
KEY, ROT_KEY, STEP = 0x9e3779b9, 0xdeadbeef, 7


def half_input(dt, f32_values):
    """``(bits, upcast)``: the values rounded to ``dt`` as uint16 bits (numpy
    float16 for fp16), and their exact float32 upcast."""
    t = torch.from_numpy(np.asarray(f32_values, F)).to(getattr(torch, dt))
    bits = t.view(torch.int16).numpy().view(np.uint16)
    return (bits.view(np.float16) if dt == "float16" else bits), t.float().numpy()


def define_compress(g, fmt, kind, bf16, r=None):
    """The wire's definition: ``(payload, r')``, ``r'`` None for the stateless wires."""
    if kind == "ef":
        return mx.compress(g, np.zeros(g.size, F) if r is None else r, fmt, bf16)
    return mx_sr.compress(g, fmt, KEY, STEP, kind == "rht", ROT_KEY, bf16), None


def define_fold(payloads, n, fmt, kind, divisor, out_dtype):
    return mx_sr.fold(payloads, n, fmt, divisor, kind == "rht", ROT_KEY, STEP, out_dtype)


@dtypes
@wires
def test_half_input_is_its_upcast(fmt, kind, dt):
    rng = np.random.default_rng(1)
    v = rng.standard_normal(1000) * np.repeat(np.exp2(rng.integers(-20, 15, 32)), 32)[:1000]
    v[40], v[100] = np.inf, np.nan
    g, up = half_input(dt, v)
    r = (rng.standard_normal(1000) * 0.01).astype(F)
    got, want = (define_compress(x, fmt, kind, b, r) for x, b in ((g, dt == "bfloat16"), (up, False)))
    assert np.array_equal(got[0], want[0])
    assert kind != "ef" or np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


# sources s0, s1, s2 of one element a block (the rest 0) and the bits of their sum
HAND = {
    "float16": [((1, 2.0 ** -11, 0), 0x3c00),                    # a tie, down to even
                ((1, 2.0 ** -10, 2.0 ** -11), 0x3c02),           # a tie, up to even
                ((2.0 ** 15, 2.0 ** 15, 0), 0x7c00),             # past 65504: infinity
                ((2.0 ** -23, 2.0 ** -24, 0), 0x0003),           # a subnormal
                ((1, np.inf, 0), 0x7e00)],                       # a NaN block
    "bfloat16": [((1, 2.0 ** -8, 0), 0x3f80),
                 ((1, 2.0 ** -7, 2.0 ** -8), 0x3f82),
                 ((1.75 * 2.0 ** 127, 1.75 * 2.0 ** 124, 1.75 * 2.0 ** 121), 0x7f80),
                 ((2.0 ** -130, 2.0 ** -131, 0), 0x000c),
                 ((1, np.inf, 0), 0x7fc0)],
}


@dtypes
def test_fold_converts_the_float32_sum_once(dt):
    srcs = np.zeros((3, 32 * len(HAND[dt])), F)
    for b, (values, _) in enumerate(HAND[dt]):
        srcs[:, 32 * b] = values
    pays = [mx.compress(s, np.zeros(s.size, F), "fp8")[0] for s in srcs]
    out = mx.fold(pays, srcs.shape[1], "fp8", 1, dt)
    assert out.dtype == (np.float16 if dt == "float16" else np.uint16)
    assert [hex(x) for x in out.view(np.uint16)[::32]] == [hex(w) for _, w in HAND[dt]]
    assert not out.view(np.uint16)[1:32].any()
    nan = np.array([0xffc12345, 0x7f800001], np.uint32).view(F)      # the casts' NaN bits
    want = [0xfe09, 0x7e00] if dt == "float16" else [0xffc1, 0x7fc0]
    assert mx.narrow(nan, dt).view(np.uint16).tolist() == want


@dtypes
@wires
def test_host_path_is_the_definition_and_ctx_keeps_the_dtype(fmt, kind, dt):
    comp, bf16 = COMP[fmt, kind], dt == "bfloat16"
    g, _ = half_input(dt, np.random.default_rng(2).standard_normal(100) * 3)
    t = torch.from_numpy(g.view(np.int16).copy()).view(getattr(torch, dt))
    assert comp.compresses(t) and comp.compresses(np.zeros(3, np.float16))
    assert not comp.compresses(np.zeros(3, np.uint16))
    if kind == "ef":
        assert comp.residual_like(t).dtype == torch.float32
        payload, ctx = comp.compress(t)
    else:
        payload, ctx = comp.compress(t, KEY, STEP, ROT_KEY)
    want = define_compress(g, fmt, kind, bf16)[0]
    assert np.array_equal(payload.numpy(), want)
    out = comp.decompress(payload, ctx)
    assert out.dtype == t.dtype and out.shape == t.shape
    assert np.array_equal(out.view(torch.int16).numpy().view(np.uint16),
                          define_fold([want], 100, fmt, kind, 1, dt).view(np.uint16))
    if not bf16:                                                      # numpy float16 counts too
        assert np.array_equal(comp.compress(g, *(() if kind == "ef" else (KEY, STEP, ROT_KEY)))[0],
                              want)


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_typed_creates_check_operands_before_any_device_call(fmt):
    red = reducer.GpuReducer()
    A, R, P, H = 0x10000, 0x20000, 0x30000, DType.FLOAT16
    for dtype in (DType.FLOAT64, DType.INT32, 7):
        for make in (lambda: red.mx_plan([(A, R, P, 64)], fmt, dtype),
                     lambda: red.mx_fold_plan([(A, [P], 64)], 1, fmt, dtype),
                     lambda: red.mx_sr_plan([(A, P, 64, 1, 2)], fmt, True, dtype),
                     lambda: red.mx_rht_fold_plan([(A, [P], 64, 2)], 1, fmt, dtype)):
            with pytest.raises(reducer.ReduceError) as e:
                make()
            assert e.value.code == reducer.EDTYPE
    bad = [lambda: red.mx_plan([(A + 1, R, P, 64)], fmt, H),             # an odd address
           lambda: red.mx_plan([(A, R + 2, P, 64)], fmt, H),             # the residual's 4 bytes
           lambda: red.mx_plan([(A, A + 64, P, 64)], fmt, H),            # inside the 128-byte gradient
           lambda: red.mx_plan([(A, R, P, 64), (A + 126, R + 256, P + 4096, 64)], fmt, H),
           lambda: red.mx_sr_plan([(A + 1, P, 64, 1, 2)], fmt, False, DType.BFLOAT16),
           lambda: red.mx_sr_plan([(P + 16, P, 64, 1, 2)], fmt, False, H),
           lambda: red.mx_fold_plan([(A + 3, [P], 64)], 1, fmt, H),
           lambda: red.mx_fold_plan([(P + 32, [P], 64)], 1, fmt, H),
           lambda: red.mx_rht_fold_plan([(A + 1, [P], 64, 2)], 1, fmt, DType.BFLOAT16),
           lambda: red.mx_rht_fold_plan([(A, [P], 64, 2), (A + 100, [P + 4096], 64, 2)], 1, fmt, H)]
    for make in bad:
        with pytest.raises(reducer.ReduceError) as e:
            make()
        assert e.value.code == reducer.EARGS
    # FLOAT32 through a typed create is the untyped plan: the same answers
    lib, bits, h = red.lib, mx.bits_of(fmt), ctypes.c_void_p()
    desc = (reducer.MXDesc * 1)()
    for d in (DType.FLOAT32, H, DType.BFLOAT16):
        assert lib.byteps_reduce_mx_plan_create_typed(desc, 0, bits, d, ctypes.byref(h)) == 0
        assert lib.byteps_reduce_mx_plan_destroy(h) == 0             # no segments: no table
    desc[0].grad, desc[0].resid, desc[0].payload, desc[0].nelem = A + 2, R, P, 64
    assert lib.byteps_reduce_mx_plan_create(desc, 1, bits, ctypes.byref(h)) == reducer.EARGS
    assert lib.byteps_reduce_mx_plan_create_typed(desc, 1, bits, 0, ctypes.byref(h)) == reducer.EARGS
    assert lib.byteps_reduce_version() == 5
