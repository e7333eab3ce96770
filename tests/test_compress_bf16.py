"""BF16 gradient compression without a GPU: ``Compression.bf16`` on host
tensors and numpy arrays (torch's CPU casts are the semantics the kernels are
pinned to), ``Worker`` with a bf16-compressed context over a stub front end
(size, dtype, partitions and request word of the COMPRESSED tensor), and the
argument checks of byteps_reduce_compress_to / _decompress_from /
_cast_plan_create_wire, all made before any HIP call."""
import ctypes

import numpy as np
import pytest

from prophet_amd import reducer
from prophet_amd.buckets import depair_command
from prophet_amd.compression import (BF16Compressor, CastPlanCache, Compression, Compressor,
                                     FP16Compressor)
from prophet_amd.dtypes import DType
from prophet_amd.pushpull import Worker

torch = pytest.importorskip("torch")

A, B, C, D = 0x10000, 0x80000, 0x100000, 0x180000   # never dereferenced
F16, BF16 = int(DType.FLOAT16), int(DType.BFLOAT16)
WIDE_BF16 = (DType.FLOAT32, DType.FLOAT64, DType.FLOAT16)


def _all_bf16():
    return torch.from_numpy(np.arange(1 << 16, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


def _bits16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def test_compresses_and_pass_through():
    assert Compression.bf16 is BF16Compressor and issubclass(BF16Compressor, Compressor)
    assert BF16Compressor.WIRE_DTYPE == DType.BFLOAT16
    assert FP16Compressor.WIRE_DTYPE == DType.FLOAT16
    for dt in (torch.float32, torch.float64, torch.float16):
        assert Compression.bf16.compresses(torch.zeros(3, dtype=dt))
    for a in (np.zeros(3, np.float32), np.zeros(3, np.float64), np.zeros(3, np.float16)):
        assert Compression.bf16.compresses(a)
    same = (torch.zeros(3, dtype=torch.bfloat16), torch.arange(10),
            torch.arange(10, dtype=torch.uint8), np.arange(5), np.arange(5, dtype=np.uint16))
    for x in same:
        assert not Compression.bf16.compresses(x)
        c, ctx = Compression.bf16.compress(x)
        assert c is x and ctx == x.dtype                 # untouched, the same object
        assert Compression.bf16.decompress(c, ctx) is x


def test_compress_and_decompress_on_host_tensors_and_numpy():
    g = torch.Generator().manual_seed(3)
    for dt in (torch.float32, torch.float64, torch.float16):
        x = (torch.randn(1000, generator=g) * 300).to(dt)
        c, ctx = Compression.bf16.compress(x)
        assert ctx == dt and c.dtype == torch.bfloat16
        assert np.array_equal(_bits16(c), _bits16(x.to(torch.bfloat16)))
        back = Compression.bf16.decompress(c, ctx)
        assert back.dtype == dt and torch.equal(back, c.to(dt))
    a = np.linspace(-3e38, 3e38, 77, dtype=np.float32)
    c, ctx = Compression.bf16.compress(a)
    assert isinstance(c, np.ndarray) and c.dtype == np.uint16 and ctx == np.float32
    assert np.array_equal(c, _bits16(torch.from_numpy(a).to(torch.bfloat16)))
    back = Compression.bf16.decompress(c, ctx)
    assert back.dtype == np.float32
    assert np.array_equal(back, (c.astype(np.uint32) << 16).view(np.float32))


def test_into_round_trip_on_the_host():
    # the pinned f32 -> bf16 cases: subnormals kept, ties to even, the overflow edge, zeros
    xb = np.array([0x00008001, 0x00008000, 0x007fffff, 0x7f7f8000, 0x7f7f7fff, 0xff7f8000,
                   0x00000000, 0x80000000, 0x3f808000, 0x3f818000], np.uint32)
    want = [0x0001, 0x0000, 0x0080, 0x7f80, 0x7f7f, 0xff80, 0x0000, 0x8000, 0x3f80, 0x3f82]
    x = torch.from_numpy(xb.view(np.float32).copy())
    wire = BF16Compressor.wire_like(x)
    assert wire.dtype == torch.bfloat16 and wire.numel() == x.numel()
    assert Compression.bf16.compress_into(wire, x) is wire
    assert _bits16(wire).tolist() == want
    out = torch.empty_like(x)
    assert Compression.bf16.decompress_into(out, wire) is out
    assert out.view(torch.int32).tolist() == [w << 16 if w < 0x8000 else (w << 16) - (1 << 32)
                                              for w in want]
    # numpy: the wire buffer is raw uint16 bits
    xn = xb.view(np.float32).copy()
    wn = BF16Compressor.wire_like(xn)
    assert wn.dtype == np.uint16
    assert Compression.bf16.compress_into(wn, xn) is wn and wn.tolist() == want
    on = np.empty_like(xn)
    Compression.bf16.decompress_into(on, wn, 1)
    assert np.array_equal(on.view(np.uint32), np.array(want, np.uint32) << 16)
    # many_into on host tensors: the per-tensor calls, no plan built
    cache = CastPlanCache()
    w2 = [BF16Compressor.wire_like(x), BF16Compressor.wire_like(xn)]
    assert Compression.bf16.compress_many_into(w2, [x, xn], plans=cache) is w2
    assert _bits16(w2[0]).tolist() == want and w2[1].tolist() == want
    o2 = [torch.empty_like(x), np.empty_like(xn)]
    Compression.bf16.decompress_many_into(o2, w2, 3, plans=cache)
    one = Compression.bf16.decompress_into(torch.empty_like(x), wire, 3)
    assert torch.equal(o2[0].view(torch.int32), one.view(torch.int32))
    assert np.array_equal(o2[1].view(np.uint32), one.numpy().view(np.uint32))
    assert len(cache) == 0 and cache.built == 0
    with pytest.raises(ValueError):
        Compression.bf16.decompress_into(out, wire, 0)
    with pytest.raises(ValueError):
        Compression.bf16.compress_many_into(w2[:1], [x, xn])


def test_f64_is_rounded_through_f32():
    t = 1 + 2.0 ** -8 + 2.0 ** -40          # a direct f64 -> bf16 rounding would give 0x3f81
    x = torch.tensor([t, -t, 1e-40, -1e-40, 3.4028235677973366e38, 3.39e38], dtype=torch.float64)
    c, ctx = Compression.bf16.compress(x)
    assert ctx == torch.float64
    assert _bits16(c).tolist() == [0x3f80, 0xbf80, 0x0001, 0x8001, 0x7f80, 0x7f7f]
    cn, _ = Compression.bf16.compress(x.numpy())
    assert cn.tolist() == [0x3f80, 0xbf80, 0x0001, 0x8001, 0x7f80, 0x7f7f]


def test_decompress_into_divides_before_widening():
    b = _all_bf16()
    fin = ~torch.isnan(b)
    for dt in (torch.float32, torch.float64, torch.float16):
        out = torch.empty(b.numel(), dtype=dt)
        assert Compression.bf16.decompress_into(out, b, 3) is out
        want = b.clone().div_(3).to(dt)
        assert torch.equal(out[fin], want[fin]) and bool(torch.isnan(out[~fin]).all())
    after = b.to(torch.float32) / 3                     # the wrong order: widen, then divide
    out = Compression.bf16.decompress_into(torch.empty(b.numel()), b, 3)
    assert int((out[fin] != after[fin]).sum()) == 43350
    # the formula of the kernel: bf16_rne(float(b) / float(d)), f32 subnormal quotients kept
    for d in (2, 3, 7, 8, 16):
        q = (b.to(torch.float32) / float(d)).to(torch.bfloat16)
        got = b.clone().div_(d)
        assert torch.equal(got[fin].view(torch.int16), q[fin].view(torch.int16)), d


class StubFrontend:
    """One worker's front end: records every request word, answers a pull with
    the key's last push."""

    size = 1

    def __init__(self):
        self.log, self.store = [], {}

    def push(self, cmd, key, worker, data, nbytes):
        self.log.append((depair_command(cmd), key, nbytes))
        self.store[key] = np.asarray(data).view(np.uint8).copy()
        assert self.store[key].nbytes == nbytes

    def pull(self, key, out, nbytes):
        np.asarray(out).view(np.uint8)[:] = self.store[key]


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_worker_context_is_the_compressed_tensor(kind):
    n = 2 * 500 + 77
    fe = StubFrontend()
    w = Worker(0, fe, partition_bytes=1000)
    wrap = (lambda a: a) if kind == "numpy" else torch.from_numpy
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-130, 120, n))).astype(np.float32)
    x[:4] = [7e4, -65520.0, 1e-40, -0.0]
    w.declare("g")
    ctx = w.init_tensor("g", wrap(np.zeros(n, np.float32)), DType.FLOAT32,
                        compression=Compression.bf16)
    assert ctx.compressor is BF16Compressor
    assert ctx.dtype == DType.BFLOAT16 and ctx.size == 2 * n
    assert ctx.orig_dtype == DType.FLOAT32 and ctx.orig_size == 4 * n
    assert [ln for _, _, ln in ctx.parts] == [1000, 1000, 154] and ctx.key_list == [0, 1, 2]
    out = wrap(np.full(n, 123.0, np.float32))
    w.push_pull("g", wrap(x.copy()), output=out, average=False)
    assert len(fe.log) == 6 and all(req == (0, 11) for req, _, _ in fe.log)
    assert [nb for _, _, nb in fe.log] == [1000, 1000, 154] * 2
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(np.asarray(out).view(np.uint32), want.view(np.uint32))
    assert np.isfinite(np.asarray(out)[:2]).all()        # fp16 would have made these inf
    # a bf16 tensor passes through; broadcast and a foreign tensor are refused
    w.declare("b")
    cb = w.init_tensor("b", torch.zeros(300, dtype=torch.bfloat16), DType.BFLOAT16,
                       compression=Compression.bf16)
    assert cb.compressor is None and cb.size == 600
    with pytest.raises(ValueError):
        w.broadcast("g", wrap(x.copy()), root_rank=0)
    with pytest.raises(ValueError):
        w.push_pull("g", np.arange(n, dtype=np.float64))
    # one iteration over an fp16 and a bf16 context on the host: no plans
    w.declare("h")
    w.init_tensor("h", wrap(np.zeros(n, np.float32)), DType.FLOAT32, compression=Compression.fp16)
    held = {"g": wrap(x.copy()), "h": wrap(x.copy())}
    w.push_pull_iteration(held, average=True)
    assert np.array_equal(np.asarray(held["g"]).view(np.uint32), want.view(np.uint32))
    wanth = torch.from_numpy(x).to(torch.float16).to(torch.float32).numpy()
    assert np.array_equal(np.asarray(held["h"]).view(np.uint32), wanth.view(np.uint32))
    assert np.isinf(np.asarray(held["h"])[0]) and len(w._cast_plans) == 0
    w.close()


@pytest.fixture(scope="module")
def lib():
    return reducer.load_library()


def _segs(*triples):
    arr = (reducer.CastDesc * max(1, len(triples)))()
    for i, (w, h, n) in enumerate(triples):
        arr[i].wide, arr[i].half, arr[i].nelem = w, h, n
    return arr


def test_one_tensor_argument_errors_without_a_gpu(lib):
    comp, decomp = lib.byteps_reduce_compress_to, lib.byteps_reduce_decompress_from
    bad_pairs = [(dt, BF16) for dt in (DType.INT32, DType.UINT8, DType.INT64, DType.INT8,
                                       DType.BFLOAT16, 7, -1)]
    bad_pairs += [(dt, F16) for dt in (DType.INT32, DType.FLOAT16, 7)]
    bad_pairs += [(DType.FLOAT32, w) for w in (DType.FLOAT32, DType.FLOAT64, DType.INT32, 7, -1)]
    for dt, wire in bad_pairs:
        assert comp(A, B, 64, int(dt), int(wire), None) == reducer.EDTYPE, (dt, wire)
        assert decomp(A, B, 64, int(dt), int(wire), 1, None) == reducer.EDTYPE, (dt, wire)
        assert b"data type" in lib.byteps_reduce_last_error()
    pairs = [(dt, BF16) for dt in WIDE_BF16]
    pairs += [(dt, F16) for dt in (DType.FLOAT32, DType.FLOAT64, DType.BFLOAT16)]
    for dt, wire in pairs:
        dt = int(dt)
        assert comp(None, B, 64, dt, wire, None) == reducer.EARGS
        assert comp(A, None, 64, dt, wire, None) == reducer.EARGS
        assert decomp(None, B, 64, dt, wire, 1, None) == reducer.EARGS
        assert decomp(A, None, 64, dt, wire, 1, None) == reducer.EARGS
        assert decomp(A, B, 64, dt, wire, 0, None) == reducer.EARGS
        assert decomp(A, B, 64, dt, wire, -3, None) == reducer.EARGS
        assert comp(A, A, 64, dt, wire, None) == reducer.EARGS          # overlap
        assert decomp(A + 127, A, 64, dt, wire, 1, None) == reducer.EARGS
        # nothing to do: no launch, no pointer needed
        assert comp(None, None, 0, dt, wire, None) == reducer.OK
        assert decomp(None, None, 0, dt, wire, 4, None) == reducer.OK
    assert comp(A, B, ctypes.c_size_t(-1).value // 2, int(DType.FLOAT64), BF16,
                None) == reducer.EARGS
    assert lib.byteps_reduce_version() == 5


def test_plan_argument_errors_without_a_gpu(lib):
    def create(triples, dt, wire, nsegs=None):
        out = ctypes.c_void_p(0x1234)
        rc = lib.byteps_reduce_cast_plan_create_wire(
            _segs(*triples), len(triples) if nsegs is None else nsegs, int(dt), int(wire),
            ctypes.byref(out))
        return rc, out

    for dt, wire in [(DType.BFLOAT16, BF16), (DType.FLOAT16, F16), (DType.INT32, BF16),
                     (DType.INT64, F16), (7, BF16), (DType.FLOAT32, DType.FLOAT32),
                     (DType.FLOAT32, DType.FLOAT64), (DType.FLOAT32, -1)]:
        rc, out = create([(A, B, 64)], dt, wire)
        assert rc == reducer.EDTYPE and not out.value, (dt, wire)
        assert b"data type" in lib.byteps_reduce_last_error()
    for dt, wire in [(d, BF16) for d in WIDE_BF16] + [(DType.FLOAT32, F16), (DType.BFLOAT16, F16)]:
        assert create([(A, B, 64), (None, D, 8)], dt, wire)[0] == reducer.EARGS
        rc, out = create([(A, B, 64), (C, None, 8)], dt, wire)
        assert rc == reducer.EARGS and not out.value          # the out-pointer is cleared
        assert create([(A, B, 64)], dt, wire, nsegs=-1)[0] == reducer.EARGS
        assert lib.byteps_reduce_cast_plan_create_wire(
            None, 2, int(dt), wire, ctypes.byref(ctypes.c_void_p())) == reducer.EARGS
        assert lib.byteps_reduce_cast_plan_create_wire(_segs((A, B, 64)), 1, int(dt), wire,
                                                       None) == reducer.EARGS
        assert create([(A, B, 100), (C, B + 198, 100)], dt, wire)[0] == reducer.EARGS
        assert b"overlap" in lib.byteps_reduce_last_error()
        assert create([(A, B, ctypes.c_size_t(-1).value // 2)], dt, wire)[0] == reducer.EARGS


def test_reducer_bounds_checks_precede_the_call(monkeypatch):
    red = reducer.GpuReducer()
    called = []
    for name in ("byteps_reduce_compress_to", "byteps_reduce_decompress_from",
                 "byteps_reduce_cast_plan_create_wire", "byteps_reduce_cast_plan_create"):
        monkeypatch.setattr(red.lib, name,
                            lambda *a, name=name: called.append(name) or reducer.EARGS)
    wire = torch.empty(99, dtype=torch.bfloat16)
    wide = torch.empty(100, dtype=torch.float32)
    full = torch.empty(100, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        red.compress(wire, wide, 100, DType.FLOAT32, DType.BFLOAT16)      # dst one element short
    with pytest.raises(ValueError):
        red.decompress(wide, wire, 100, DType.FLOAT32, DType.BFLOAT16)    # src one element short
    with pytest.raises(ValueError):
        red.decompress(wide[:99], full, 100, DType.FLOAT32, DType.BFLOAT16, 2)
    with pytest.raises(ValueError):
        red.compress(full, wide, 100, DType.FLOAT64, DType.BFLOAT16)      # 400 bytes: 50 doubles
    with pytest.raises(ValueError):
        red.compress(full, torch.empty(99, dtype=torch.float16), 100, DType.FLOAT16,
                     DType.BFLOAT16)
    with pytest.raises(ValueError):
        red.cast_plan([(wide, wire, 100)], DType.FLOAT32, DType.BFLOAT16)
    assert not called
    with pytest.raises(reducer.ReduceError):                              # in bounds: asked
        red.cast_plan([(wide, full, 100)], DType.FLOAT32, DType.BFLOAT16)
    assert called == ["byteps_reduce_cast_plan_create_wire"]
    with pytest.raises(reducer.ReduceError):                              # the default wire: fp16
        red.cast_plan([(wide, full, 100)], DType.FLOAT32)
    assert called[-1] == "byteps_reduce_cast_plan_create"
    with pytest.raises(reducer.ReduceError):
        red.compress(full, wide, 100, DType.FLOAT32, DType.BFLOAT16)
    assert called[-1] == "byteps_reduce_compress_to"
