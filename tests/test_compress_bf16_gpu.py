"""The bf16 cast kernels (prophet_amd/csrc/bpsr_k_cast_bf16.hip) on the GPU
against the host: CPU torch casts and CPU ``Tensor.div_`` on a bf16 tensor.
Bits are compared everywhere except where the expected value is a NaN; there
only a NaN is required (the payload is not part of the contract).  The
all-patterns decompress is the case that catches a flushed f32 denormal (a
bf16 quotient can be an f32 subnormal) and a widen-first divide."""
import numpy as np
import pytest

from prophet_amd import reducer
from prophet_amd.dtypes import DType, from_torch
from prophet_amd.reducer import GpuReducer

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

BF = DType.BFLOAT16
WIDE = [torch.float32, torch.float64, torch.float16]
IDS = ["f32", "f64", "f16"]
BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32,
        torch.float64: torch.int64}
# Launches this short run tiles of 256 lanes x 8 elements x 1 unit per lane
# (tests/test_compress_gpu.py's TILE).
TILE = 256 * 8


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return GpuReducer(device=0)


def _bits(t):
    return t.contiguous().view(BITS[t.dtype])


def _mismatches(got, want) -> int:
    """Elements of ``got`` (any device) that differ from the host's ``want``:
    other bits where want is a number, not a NaN where want is one."""
    got = got.cpu()
    nan = torch.isnan(want)
    bad = (_bits(got) != _bits(want)) & ~nan
    bad |= nan & ~torch.isnan(got)
    return int(bad.sum())


def _all_bf16():
    return torch.from_numpy(np.arange(1 << 16, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)


@pytest.fixture(scope="module")
def quotients():
    """The host's ``b.div_(d)`` over every bf16 pattern, computed once."""
    b = _all_bf16()
    return b, {d: (b.clone().div_(d) if d > 1 else b) for d in (1, 2, 3, 7, 16)}


@pytest.mark.parametrize("dt", WIDE, ids=IDS)
def test_decompress_every_bf16_pattern(red, quotients, dt):
    b, q = quotients
    bd = b.cuda()
    for d in (1, 2, 3, 7, 16):
        want = q[d].to(dt)
        out = torch.empty(b.numel(), dtype=dt, device="cuda")
        red.decompress(out, bd, b.numel(), from_torch(dt), BF, d)
        assert _mismatches(out, want) == 0, (dt, d)
    if dt == torch.float32:
        fin = ~torch.isnan(b)
        # the input tells divide-then-widen from widen-then-divide apart ...
        out3 = torch.empty(b.numel(), device="cuda")
        red.decompress(out3, bd, b.numel(), DType.FLOAT32, BF, 3)
        assert int((out3.cpu()[fin] != (b.float() / 3)[fin]).sum()) == 43350
        # ... and holds the quotients that a flushed denormal would turn into zero
        f = b.float() / 3
        sub = fin & (f != 0) & (f.abs() < 2.0 ** -126)
        assert int(sub.sum()) == 638
        assert int((q[3].float()[sub] != 0).sum()) > 600


def _structured_f32():
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    lows = np.array([0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff], np.uint32)
    grid = (hi[:, None] | lows[None, :]).reshape(-1)
    rng = np.random.default_rng(20)
    rnd = rng.standard_normal(1 << 20) * np.exp2(rng.uniform(-140.0, 127.0, 1 << 20))
    with np.errstate(over="ignore"):
        rnd = rnd.astype(np.float32)
    return torch.from_numpy(np.concatenate([grid.view(np.float32), rnd]))


def test_compress_f32_every_tie_neighbour_and_random(red):
    x = _structured_f32()
    assert x.numel() == 393216 + (1 << 20)
    want = x.to(torch.bfloat16)
    w = _bits(want).numpy().view(np.uint16)
    xb = x.view(torch.int32).numpy().view(np.uint32)
    # the host is the pinned semantics: subnormals kept, ties to even, the overflow edge
    for src, dst in [(0x00008001, 0x0001), (0x00008000, 0x0000), (0x007fffff, 0x0080),
                     (0x7f7f8000, 0x7f80), (0x7f7f7fff, 0x7f7f), (0x80000000, 0x8000),
                     (0xff7f8000, 0xff80), (0x3f818000, 0x3f82)]:
        assert (w[xb == src] == dst).all() and (xb == src).any(), hex(src)
    out = torch.empty(x.numel(), dtype=torch.bfloat16, device="cuda")
    red.compress(out, x.cuda(), x.numel(), DType.FLOAT32, BF)
    assert _mismatches(out, want) == 0
    assert int(((w & 0x7f80) == 0).sum()) > 2000              # subnormal results are in the set
    assert int(torch.isinf(want).sum()) >= 6 and int(torch.isnan(want).sum()) > 700


def test_compress_f64_and_f16(red):
    g = torch.Generator().manual_seed(21)
    x64 = torch.randn(1 << 16, generator=g, dtype=torch.float64) * \
        torch.exp2(torch.randint(-150, 128, (1 << 16,), generator=g).double())
    t = 1 + 2.0 ** -8 + 2.0 ** -40                           # through f32: 1.0, direct: 0x3f81
    named = [t, -t, 1e-40, -1e-40, 3.4028235677973366e38, 3.39e38, float("nan"), float("inf"),
             1e-300, -0.0]
    x64[:len(named)] = torch.tensor(named, dtype=torch.float64)
    want = x64.to(torch.bfloat16)
    assert _bits(want).numpy().view(np.uint16)[:6].tolist() == [0x3f80, 0xbf80, 0x0001, 0x8001,
                                                                 0x7f80, 0x7f7f]
    out = torch.empty(x64.numel(), dtype=torch.bfloat16, device="cuda")
    red.compress(out, x64.cuda(), x64.numel(), DType.FLOAT64, BF)
    assert _mismatches(out, want) == 0
    xh = torch.from_numpy(np.arange(1 << 16, dtype=np.uint16).view(np.float16))
    want = xh.to(torch.bfloat16)
    out = torch.empty(xh.numel(), dtype=torch.bfloat16, device="cuda")
    red.compress(out, xh.cuda(), xh.numel(), DType.FLOAT16, BF)
    assert _mismatches(out, want) == 0


GUARD = 64          # bytes
SIZES = (1, 7, 8, 9, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
OFFS = (0, 1, 3, 4)  # elements: heads, tails, and pairs that never co-align


def _aligned_bytes(nbytes):
    """A device byte buffer whose first byte is 256-byte aligned."""
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    skip = (-raw.data_ptr()) % 256
    return raw[skip:skip + nbytes]


@pytest.mark.parametrize("compress", [True, False], ids=["compress", "decompress"])
@pytest.mark.parametrize("dt", WIDE, ids=IDS)
def test_geometry_offsets_tails_and_guards(red, dt, compress):
    """Every size around the tile and the 8-element unit, dst and src offset
    independently from a 256-byte-aligned base (pairs that co-align after a
    head, pairs that never do), guard bytes on both sides of dst intact."""
    nmax = max(SIZES)
    g = torch.Generator().manual_seed(22)
    src_dt, dst_dt = (dt, torch.bfloat16) if compress else (torch.bfloat16, dt)
    base = (torch.randn(nmax, generator=g) * 100).to(src_dt)
    divisor = 1 if compress else 3
    want = base.to(torch.bfloat16) if compress else base.clone().div_(divisor).to(dt)
    want_d = _bits(want).cuda()
    ses, des = base.element_size(), want.element_size()
    sbuf = _aligned_bytes((nmax + max(OFFS)) * ses)
    dbuf = _aligned_bytes(256 + (nmax + max(OFFS)) * des + GUARD)
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    for so in OFFS:
        src = sbuf[so * ses:(so + nmax) * ses].view(src_dt)
        src.copy_(base)
        for do in OFFS:
            for n in SIZES:
                dbuf.fill_(0xA5)
                d0 = 256 + do * des                       # >= GUARD bytes before dst
                dst = dbuf[d0:d0 + n * des].view(dst_dt)
                if compress:
                    red.compress(dst, src, n, from_torch(dt), BF)
                else:
                    red.decompress(dst, src, n, from_torch(dt), BF, divisor)
                bad += (dst.view(BITS[dst_dt]) != want_d[:n]).sum()
                bad += (dbuf[d0 - GUARD:d0] != 0xA5).sum()
                bad += (dbuf[d0 + n * des:d0 + n * des + GUARD] != 0xA5).sum()
    assert not bool(torch.isnan(want).any())
    assert int(bad) == 0


def test_two_unit_tiles_and_nt_stores(red):
    """The sizes where the launch shape changes: 2 units per lane from 2048
    tiles on (8 Mi elements), non-temporal stores from 96 MiB of output on
    (48 Mi bf16 elements; 24 Mi f32 elements) — odd lengths, an unaligned head."""
    g = torch.Generator(device="cuda").manual_seed(23)
    n = (48 << 20) + 3 * 4096 + 13
    buf = torch.randn(n + 4, generator=g, device="cuda")
    x = buf[1:1 + n]                             # 4 B and 2 B past alignment: a 7-element head
    hbuf = torch.empty(n + 8, dtype=torch.bfloat16, device="cuda")
    h = hbuf[1:1 + n]
    xc = x.cpu()
    for m in (n, (8 << 20) + 4096 + 11):
        red.compress(h[:m], x[:m], m, DType.FLOAT32, BF)
        want = xc[:m].to(torch.bfloat16)
        assert torch.equal(h[:m].cpu().view(torch.int16), want.view(torch.int16)), m
        out = torch.empty(m + 4, device="cuda")[1:1 + m]
        red.decompress(out, h[:m], m, DType.FLOAT32, BF, 3)
        wantw = want.div_(3).float()
        assert torch.equal(out.cpu().view(torch.int32), wantw.view(torch.int32)), m


def test_short_operands_and_bad_pairs_raise_before_any_launch(red):
    wide = torch.zeros(1000, device="cuda")
    wire = torch.zeros(999, dtype=torch.bfloat16, device="cuda")
    full = torch.zeros(1000, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        red.compress(wire, wide, 1000, DType.FLOAT32, BF)                 # dst one element short
    with pytest.raises(ValueError):
        red.decompress(wide[:999], full, 1000, DType.FLOAT32, BF, 2)      # dst one element short
    with pytest.raises(ValueError):
        red.decompress(wide, wire, 1000, DType.FLOAT32, BF)               # src one element short
    other = torch.zeros(1000, dtype=torch.bfloat16, device="cuda")
    ints = torch.zeros(1000, dtype=torch.int32, device="cuda")
    for src, dt, wire_dt in [(other, BF, BF), (ints, DType.INT32, BF),
                             (wide, DType.FLOAT32, DType.FLOAT32),
                             (wide, DType.FLOAT32, DType.INT32)]:
        with pytest.raises(reducer.ReduceError) as e:
            red.compress(full, src, 1000, dt, wire_dt)
        assert e.value.code == reducer.EDTYPE
        with pytest.raises(reducer.ReduceError) as e:
            red.decompress(src, full, 1000, dt, wire_dt, 2)
        assert e.value.code == reducer.EDTYPE
    torch.cuda.synchronize()
    assert float(wide.abs().sum()) == 0.0 and float(full.float().abs().sum()) == 0.0
    assert float(wire.float().abs().sum()) == 0.0 and int(ints.abs().sum()) == 0


def test_fp16_wire_through_the_new_calls_is_the_fp16_cast(red):
    g = torch.Generator().manual_seed(24)
    x = (torch.randn(3 * TILE + 5, generator=g) * 3e4).cuda()
    a = torch.empty(x.numel(), dtype=torch.float16, device="cuda")
    b = torch.empty_like(a)
    red.compress_fp16(a, x, x.numel(), DType.FLOAT32)
    red.compress(b, x, x.numel(), DType.FLOAT32, DType.FLOAT16)
    assert torch.equal(_bits(a), _bits(b)) and bool(torch.isinf(a).any())
    oa, ob = torch.empty_like(x), torch.empty_like(x)
    red.decompress_fp16(oa, a, x.numel(), DType.FLOAT32, 3)
    red.decompress(ob, a, x.numel(), DType.FLOAT32, DType.FLOAT16, 3)
    assert torch.equal(_bits(oa), _bits(ob))


def test_torch_ops_opcheck_compile_and_compression(red):
    from prophet_amd import torch_ops  # noqa: F401
    from prophet_amd.compression import Compression
    x = torch.randn(4099, device="cuda") * 1e5
    want = x.cpu().to(torch.bfloat16)

    def f(t):
        h = torch.ops.bpsr.compress_bf16(t)
        out = torch.empty_like(t)
        torch.ops.bpsr.decompress_bf16_out(out, h, 3)
        return h, out * 1.0

    h, out = torch.compile(f, fullgraph=True)(x)
    assert h.dtype == torch.bfloat16
    assert torch.equal(h.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(out.cpu(), want.clone().div_(3).float())
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.bpsr.compress_bf16.default, (x,), test_utils=utils)
    torch.library.opcheck(torch.ops.bpsr.compress_bf16_out.default,
                          (torch.empty(4099, dtype=torch.bfloat16, device="cuda"), x),
                          test_utils=utils)
    torch.library.opcheck(torch.ops.bpsr.decompress_bf16_out.default,
                          (torch.empty_like(x), h, 3), test_utils=utils)
    # the Compression front end takes the same kernels for device tensors
    c, ctx = Compression.bf16.compress(x.double())
    assert ctx == torch.float64 and c.is_cuda and c.dtype == torch.bfloat16
    assert torch.equal(c.cpu().view(torch.int16),
                       x.double().cpu().to(torch.bfloat16).view(torch.int16))
    back = Compression.bf16.decompress(c, ctx)
    assert back.dtype == torch.float64 and torch.equal(back.cpu(), c.cpu().double())
    xh = x.half()
    c, ctx = Compression.bf16.compress(xh)
    assert torch.equal(c.cpu().view(torch.int16), xh.cpu().to(torch.bfloat16).view(torch.int16))
    with pytest.raises(Exception):
        torch.ops.bpsr.compress_bf16(torch.arange(8, device="cuda"))   # integers: EDTYPE
    with pytest.raises(Exception):
        torch.ops.bpsr.compress_bf16(c)                                # bf16 to bf16: EDTYPE
    with pytest.raises(Exception):
        torch.ops.bpsr.decompress_bf16_out(torch.empty_like(x), h.half(), 1)   # fp16 wire
