"""The fp16 cast kernels (prophet_amd/csrc/bpsr_k_cast.hip) on the GPU against
the host: CPU torch casts and CPU ``Tensor.div_`` on an fp16 tensor.  Bits are
compared everywhere except where the expected value is a NaN; there only a
NaN is required (the payload is not part of the contract)."""
import numpy as np
import pytest

from prophet_amd.dtypes import DType, from_torch
from prophet_amd.reducer import GpuReducer

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

WIDE = [torch.float32, torch.float64, torch.bfloat16]
IDS = ["f32", "f64", "bf16"]
BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32,
        torch.float64: torch.int64}
# Launches this short run tiles of 256 lanes x 8 elements x 1 unit per lane
# (2 units, the copy's residency, only from 2048 tiles of that size on).
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


def _all_halves():
    return torch.from_numpy(np.arange(1 << 16, dtype=np.uint16).view(np.float16))


@pytest.mark.parametrize("dt", WIDE, ids=IDS)
def test_decompress_every_f16_pattern(red, dt):
    h = _all_halves()
    hd = h.cuda()
    for d in (1, 2, 3, 7, 16):
        want = h.clone().div_(d).to(dt) if d > 1 else h.to(dt)
        out = torch.empty(h.numel(), dtype=dt, device="cuda")
        red.decompress_fp16(out, hd, h.numel(), from_torch(dt), d)
        assert _mismatches(out, want) == 0, (dt, d)
    # the input tells divide-then-widen from widen-then-divide apart
    if dt == torch.float32:
        fin = ~torch.isnan(h)
        assert int((out.cpu()[fin] != (h.float() / 16)[fin]).sum()) > 0


def _structured_f32():
    hb = np.arange(0x7c00, dtype=np.uint16)                  # every finite fp16 magnitude
    lo = hb.view(np.float16).astype(np.float64)
    hi = (hb + 1).view(np.float16).astype(np.float64)
    hi[-1] = 65536.0                                         # 65504's successor rounds to inf
    mid = ((lo + hi) / 2).astype(np.float32)                 # 12 significant bits: exact
    assert np.array_equal(mid.astype(np.float64), (lo + hi) / 2)
    inf = np.float32(np.inf)
    trio = np.concatenate([mid, np.nextafter(mid, inf), np.nextafter(mid, -inf)])
    special = np.array([65504.0, 65519.996, 65520.0, 65536.0, 1e38, 0.0, np.inf], np.float32)
    sub = np.array([1, 2, 0x7fffff, 0x400000, 0x800000], np.uint32).view(np.float32)
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0x7f801fff],
                    np.uint32).view(np.float32)
    pos = np.concatenate([trio, special, sub])
    rng = np.random.default_rng(20)
    mag = np.exp2(rng.uniform(-30.0, 17.0, 1 << 20))
    rnd = (mag * rng.choice([-1.0, 1.0], mag.size)).astype(np.float32)
    return torch.from_numpy(np.concatenate([pos, -pos, nans, rnd]))


def test_compress_f32_midpoints_neighbours_and_random(red):
    x = _structured_f32()
    assert 0x7c00 * 6 < x.numel() < (1 << 20) + (1 << 18)
    want = x.to(torch.float16)
    out = torch.empty(x.numel(), dtype=torch.float16, device="cuda")
    red.compress_fp16(out, x.cuda(), x.numel(), DType.FLOAT32)
    assert _mismatches(out, want) == 0
    w = want.view(torch.int16)
    assert int(((w & 0x7c00) == 0).sum()) > 2000             # subnormal results are in the set
    assert int(torch.isinf(want).sum()) >= 6 and int(torch.isnan(want).sum()) == 6


def test_compress_f64_and_bf16(red):
    g = torch.Generator().manual_seed(21)
    x64 = torch.randn(1 << 16, generator=g, dtype=torch.float64) * \
        torch.exp2(torch.randint(-26, 17, (1 << 16,), generator=g).double())
    t = 1 + 2.0 ** -11 + 2.0 ** -30                          # through f32: 1.0, direct: 1 + 2^-10
    x64[:6] = torch.tensor([t, -t, float("nan"), float("inf"), 65519.99999, 1e-300])
    want = x64.to(torch.float16)
    assert want.view(torch.int16)[:2].tolist() == [0x3c00, 0xbc00 - 0x10000]
    out = torch.empty(x64.numel(), dtype=torch.float16, device="cuda")
    red.compress_fp16(out, x64.cuda(), x64.numel(), DType.FLOAT64)
    assert _mismatches(out, want) == 0
    xb = torch.from_numpy(np.arange(1 << 16, dtype=np.uint16).view(np.int16)).view(torch.bfloat16)
    want = xb.to(torch.float16)
    out = torch.empty(xb.numel(), dtype=torch.float16, device="cuda")
    red.compress_fp16(out, xb.cuda(), xb.numel(), DType.BFLOAT16)
    assert _mismatches(out, want) == 0


GUARD = 64          # bytes
SIZES = (1, 7, 8, 9, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
OFFS = (0, 1, 3, 4)


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
    src_dt, dst_dt = (dt, torch.float16) if compress else (torch.float16, dt)
    base = (torch.randn(nmax, generator=g) * 100).to(src_dt)
    divisor = 1 if compress else 3
    want = base.to(torch.float16) if compress else base.clone().div_(divisor).to(dt)
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
                    red.compress_fp16(dst, src, n, from_torch(dt))
                else:
                    red.decompress_fp16(dst, src, n, from_torch(dt), divisor)
                bad += (dst.view(BITS[dst_dt]) != want_d[:n]).sum()
                bad += (dbuf[d0 - GUARD:d0] != 0xA5).sum()
                bad += (dbuf[d0 + n * des:d0 + n * des + GUARD] != 0xA5).sum()
    assert not bool(torch.isnan(want).any())
    assert int(bad) == 0


def test_two_unit_tiles_and_nt_stores(red):
    """The sizes where the launch shape changes: 2 units per lane from 2048
    tiles on (8 Mi elements), non-temporal stores from 96 MiB of output on
    (48 Mi fp16 elements; 24 Mi f32 elements) — odd lengths, an unaligned head."""
    g = torch.Generator(device="cuda").manual_seed(23)
    n = (48 << 20) + 3 * 4096 + 13
    buf = torch.randn(n + 4, generator=g, device="cuda")
    x = buf[1:1 + n]                             # 4 B and 2 B past alignment: a 7-element head
    hbuf = torch.empty(n + 8, dtype=torch.float16, device="cuda")
    h = hbuf[1:1 + n]
    xc = x.cpu()
    for m in (n, (8 << 20) + 4096 + 11):
        red.compress_fp16(h[:m], x[:m], m, DType.FLOAT32)
        want = xc[:m].to(torch.float16)
        assert torch.equal(h[:m].cpu().view(torch.int16), want.view(torch.int16)), m
        out = torch.empty(m + 4, device="cuda")[1:1 + m]
        red.decompress_fp16(out, h[:m], m, DType.FLOAT32, 3)
        wantw = want.div_(3).float()
        assert torch.equal(out.cpu().view(torch.int32), wantw.view(torch.int32)), m


def test_short_operands_raise_before_any_launch(red):
    wide = torch.zeros(1000, device="cuda")
    half = torch.zeros(999, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError):
        red.compress_fp16(half, wide, 1000, DType.FLOAT32)            # dst one element short
    with pytest.raises(ValueError):
        red.decompress_fp16(wide[:999], torch.zeros(1000, dtype=torch.float16, device="cuda"),
                            1000, DType.FLOAT32, 2)                   # dst one element short
    with pytest.raises(ValueError):
        red.decompress_fp16(wide, half, 1000, DType.FLOAT32)          # src one element short
    torch.cuda.synchronize()
    assert float(wide.abs().sum()) == 0.0 and float(half.abs().sum()) == 0.0


def test_torch_ops_opcheck_compile_and_compression(red):
    from prophet_amd import torch_ops  # noqa: F401
    from prophet_amd.compression import Compression
    x = torch.randn(4099, device="cuda") * 50
    want = x.cpu().to(torch.float16)

    def f(t):
        h = torch.ops.bpsr.compress_fp16(t)
        out = torch.empty_like(t)
        torch.ops.bpsr.decompress_fp16_out(out, h, 3)
        return h, out * 1.0

    h, out = torch.compile(f, fullgraph=True)(x)
    assert torch.equal(h.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(out.cpu(), want.clone().div_(3).float())
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.bpsr.compress_fp16.default, (x,), test_utils=utils)
    torch.library.opcheck(torch.ops.bpsr.compress_fp16_out.default,
                          (torch.empty(4099, dtype=torch.float16, device="cuda"), x),
                          test_utils=utils)
    torch.library.opcheck(torch.ops.bpsr.decompress_fp16_out.default,
                          (torch.empty_like(x), h, 3), test_utils=utils)
    # the Compression front end takes the same kernels for device tensors
    c, ctx = Compression.fp16.compress(x.double())
    assert ctx == torch.float64 and c.is_cuda
    assert torch.equal(c.cpu().view(torch.int16),
                       x.double().cpu().to(torch.float16).view(torch.int16))
    back = Compression.fp16.decompress(c, ctx)
    assert back.dtype == torch.float64 and torch.equal(back.cpu(), c.cpu().double())
    with pytest.raises(Exception):
        torch.ops.bpsr.compress_fp16(torch.arange(8, device="cuda"))   # integers: EDTYPE
