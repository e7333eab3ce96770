"""The error-feedback compress kernels (the scheme of
prophet_amd/csrc/bpsr_cast_ef.h over bpsr_cast_impl.h and bpsr_cast_single.h;
bpsr_k_cast_ef.hip, bpsr_k_cast_ef_bf16.hip) on the GPU against the host
definition in CPU torch ops:

    c = g + r;  w = wire(c);  b = w.float();  r' = where(isfinite(b), c - b, 0)

Wire bits are compared everywhere except where the expected value is a NaN
(there only a NaN is required: the payload is not part of the contract);
residual bits are compared everywhere."""
import numpy as np
import pytest

from prophet_amd import reducer
from prophet_amd.dtypes import DType
from prophet_amd.reducer import GpuReducer

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

F32 = DType.FLOAT32
WIRES = [(DType.FLOAT16, torch.float16), (DType.BFLOAT16, torch.bfloat16)]
IDS = ["fp16", "bf16"]
# Launches this short run tiles of 256 lanes x 8 elements x 1 unit per lane
TILE = 256 * 8


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return GpuReducer(device=0)


def host_ef(g, r, wire):
    """The host definition: (w, r')."""
    c = g + r
    w = c.to(wire)
    b = w.to(torch.float32)
    return w, torch.where(torch.isfinite(b), c - b, torch.zeros_like(c))


def _wire_mismatches(got, want) -> int:
    got = got.cpu()
    nan = torch.isnan(want)
    bad = (got.view(torch.int16) != want.view(torch.int16)) & ~nan
    bad |= nan & ~torch.isnan(got)
    return int(bad.sum())


def _f32(bits):
    return torch.from_numpy(np.asarray(bits, np.uint32).view(np.float32).copy())


def _specials():
    """(g, r) pairs: signed zeros, f32 subnormals, fp16 and bf16 rounding ties
    and their neighbours, the overflow boundaries of both wires, g + r
    overflowing f32, infinities and NaN — each g once with r = 0, once with a
    small and once with a large residual of either sign."""
    g = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00008000, 0x00008001,
         0x00800000,
         # fp16 ties (13 dropped bits: 0x1000 is the half) and neighbours, around 1.0
         0x3f800fff, 0x3f801000, 0x3f801001, 0x3f802fff, 0x3f803000, 0x3f803001,
         # fp16 subnormal range: 2^-25 (tie to zero), just above, 2^-24, 1.5 * 2^-24
         0x33000000, 0x33000001, 0x33800000, 0x33c00000, 0x32ffffff,
         # bf16 ties (16 dropped bits) and neighbours
         0x3f807fff, 0x3f808000, 0x3f808001, 0x3f817fff, 0x3f818000, 0x3f818001,
         # overflow boundaries: fp16 65519.99 / 65520, bf16 0x7f7f7fff / 0x7f7f8000
         0x477fdfff, 0x477fe000, 0xc77fdfff, 0xc77fe000, 0x7f7f7fff, 0x7f7f8000, 0xff7f8000,
         0x7f7fffff, 0xff7fffff,
         0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001]
    g = _f32(g)
    rs = [torch.zeros_like(g), torch.full_like(g, 2.0 ** -26), torch.full_like(g, -2.0 ** -26),
          g * 2.0 ** -12, -g * 2.0 ** -12, torch.full_like(g, 3.0e38), torch.full_like(g, -3.0e38),
          _f32([0x00000001] * g.numel()), _f32([0x80000000] * g.numel())]
    rs = [torch.where(torch.isfinite(r), r, torch.zeros_like(r)) for r in rs]
    return g.repeat(len(rs)), torch.cat(rs)


@pytest.fixture(scope="module")
def data():
    """f32 values spread over the decades with residuals of about half a wire
    ulp of the gradient in both signs (fp16: 2^-11 relative, bf16: 2^-8), and
    the block of specials.  Computed once, shared, left unchanged."""
    rng = np.random.default_rng(31)
    n = 1 << 18
    with np.errstate(over="ignore"):
        g = (rng.standard_normal(n) * np.exp2(rng.uniform(-140.0, 127.0, n))).astype(np.float32)
        rel = np.where(np.arange(n) % 2 == 0, 2.0 ** -12, 2.0 ** -9)
        r = (g * rel * rng.choice([-1.0, 1.0], n) * rng.uniform(0.9, 1.1, n)).astype(np.float32)
    r[~np.isfinite(r)] = 0
    sg, sr = _specials()
    return torch.cat([sg, torch.from_numpy(g)]), torch.cat([sr, torch.from_numpy(r)])


@pytest.mark.parametrize("wd,wt", WIRES, ids=IDS)
def test_bits_match_the_host_definition(red, data, wd, wt):
    g, r = data
    n = g.numel()
    want_w, want_r = host_ef(g, r, wt)
    assert bool(torch.isfinite(want_r).all())
    assert int(torch.isnan(want_w).sum()) >= 3 and int(torch.isinf(want_w).sum()) >= 10
    gd, rd = g.cuda(), r.cuda()
    out = torch.empty(n, dtype=wt, device="cuda")
    red.compress_ef(out, rd, gd, n, F32, wd)
    assert _wire_mismatches(out, want_w) == 0
    assert torch.equal(rd.cpu().view(torch.int32), want_r.view(torch.int32))
    assert torch.equal(gd.cpu().view(torch.int32), g.view(torch.int32))       # src untouched
    # a zero residual gives the bytes of the plain compress, but for -0.0 (sent as +0.0)
    z = torch.zeros(n, device="cuda")
    plain = torch.empty_like(out)
    red.compress_ef(out, z, gd, n, F32, wd)
    red.compress(plain, gd, n, F32, wd)
    keep = (g.view(torch.int32) != -(1 << 31)) & ~torch.isnan(g)
    assert torch.equal(out.cpu().view(torch.int16)[keep], plain.cpu().view(torch.int16)[keep])


@pytest.mark.parametrize("wd,wt", WIRES, ids=IDS)
def test_carry_over_three_calls(red, data, wd, wt):
    """Three consecutive calls over one residual with different gradients:
    the host definition iterated three times."""
    g, _ = data
    n = 5 * TILE + 77
    fin = g[torch.isfinite(g) & (g.abs() < 6e4)]
    grads = [fin[k * n:(k + 1) * n] * s for k, s in ((0, 1.0), (1, -0.5), (2, 1e-3))]
    rd = torch.zeros(n, device="cuda")
    r = torch.zeros(n)
    out = torch.empty(n, dtype=wt, device="cuda")
    for x in grads:
        red.compress_ef(out, rd, x.cuda(), n, F32, wd)
        w, r = host_ef(x, r, wt)
        assert torch.equal(out.cpu().view(torch.int16), w.view(torch.int16))
        assert torch.equal(rd.cpu().view(torch.int32), r.view(torch.int32))
    assert bool((r != 0).any())


GUARD = 64          # bytes
SIZES = (0, 1, 7, 8, 9, TILE - 1, TILE, TILE + 1, TILE + 8, 3 * TILE + 13)
F32_OFFS = (0, 1, 2, 3)     # elements: src and resid, independently
DST_OFFS = (0, 1, 4, 7)     # elements


def _aligned_bytes(nbytes):
    """A device byte buffer whose first byte is 256-byte aligned."""
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    skip = (-raw.data_ptr()) % 256
    return raw[skip:skip + nbytes]


@pytest.mark.parametrize("wd,wt", WIRES, ids=IDS)
def test_geometry_offsets_tails_and_guards(red, wd, wt):
    """Every size around the 8-element unit and the tile; src and resid offset
    independently by 0-3 elements from a 256-byte base, dst by 0, 1, 4 and 7:
    the three co-align after a head, or the residual (or the wire side) never
    co-aligns and the tensor takes the element path.  0xA5 guard bytes on both
    sides of dst and of resid stay intact."""
    nmax = max(SIZES)
    gen = torch.Generator().manual_seed(32)
    g = torch.randn(nmax, generator=gen) * 100
    r = g * 2.0 ** -10 * torch.where(torch.rand(nmax, generator=gen) < 0.5, -1.0, 1.0)
    want_w, want_r = host_ef(g, r, wt)
    ww, wr = want_w.view(torch.int16).cuda(), want_r.view(torch.int32).cuda()
    rbits = r.view(torch.int32).cuda()
    sbuf = _aligned_bytes((nmax + 4) * 4)
    rbuf = _aligned_bytes(256 + (nmax + 4) * 4 + GUARD)
    dbuf = _aligned_bytes(256 + (nmax + 8) * 2 + GUARD)
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    for so in F32_OFFS:
        src = sbuf[so * 4:(so + nmax) * 4].view(torch.float32)
        src.copy_(g)
        for ro in F32_OFFS:
            r0 = 256 + ro * 4
            for do in DST_OFFS:
                d0 = 256 + do * 2
                for n in SIZES:
                    dbuf.fill_(0xA5)
                    rbuf.fill_(0xA5)
                    res = rbuf[r0:r0 + n * 4].view(torch.int32)
                    res.copy_(rbits[:n])
                    dst = dbuf[d0:d0 + n * 2].view(wt)
                    red.compress_ef(dst, res.view(torch.float32), src, n, F32, wd)
                    bad += (dst.view(torch.int16) != ww[:n]).sum()
                    bad += (res != wr[:n]).sum()
                    bad += (dbuf[d0 - GUARD:d0] != 0xA5).sum()
                    bad += (dbuf[d0 + n * 2:d0 + n * 2 + GUARD] != 0xA5).sum()
                    bad += (rbuf[r0 - GUARD:r0] != 0xA5).sum()
                    bad += (rbuf[r0 + n * 4:r0 + n * 4 + GUARD] != 0xA5).sum()
    assert not bool(torch.isnan(want_w).any())
    assert int(bad) == 0


@pytest.mark.parametrize("which", ["src", "resid", "dst"])
def test_one_byte_misaligned_operand(red, which):
    """An operand one byte past its element alignment: every element through
    the byte-wise element path, all three operands included."""
    n = TILE + 9
    gen = torch.Generator().manual_seed(33)
    g = torch.randn(n, generator=gen) * 10
    r = g * 2.0 ** -10
    want_w, want_r = host_ef(g, r, torch.float16)
    off = {k: (1 if k == which else 0) for k in ("src", "resid", "dst")}
    sbuf = _aligned_bytes(n * 4 + 16)
    rbuf = _aligned_bytes(256 + n * 4 + 256)
    dbuf = _aligned_bytes(256 + n * 2 + 256)
    rbuf.fill_(0xA5)
    dbuf.fill_(0xA5)
    s0, r0, d0 = off["src"], 128 + off["resid"], 128 + off["dst"]
    sbuf[s0:s0 + n * 4].copy_(g.view(torch.uint8).cuda())
    rbuf[r0:r0 + n * 4].copy_(r.view(torch.uint8).cuda())
    red.compress_ef(dbuf.data_ptr() + d0, rbuf.data_ptr() + r0, sbuf.data_ptr() + s0, n, F32,
                    DType.FLOAT16, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert torch.equal(dbuf[d0:d0 + n * 2].cpu(), want_w.view(torch.uint8))
    assert torch.equal(rbuf[r0:r0 + n * 4].cpu(), want_r.view(torch.uint8))
    for buf, lo, hi in ((dbuf, d0, d0 + n * 2), (rbuf, r0, r0 + n * 4)):
        assert bool((buf[:lo] == 0xA5).all()) and bool((buf[hi:] == 0xA5).all())


@pytest.mark.parametrize("wd,wt", WIRES, ids=IDS)
def test_two_unit_tiles_and_nt_stores(red, wd, wt):
    """One case just past each threshold of the launch: 2 units per lane from
    2048 tiles on (8 Mi + 4096 + 11 elements), non-temporal stores from 96 MiB
    written on — 6 bytes an element, so 16 Mi elements — with odd lengths and
    an unaligned head (the three operands co-align after 7 elements)."""
    gen = torch.Generator(device="cuda").manual_seed(34)
    n = (16 << 20) + 3 * 4096 + 13
    assert n * 6 >= 96 << 20 > ((8 << 20) + 4096 + 11) * 6
    x = torch.randn(n + 4, generator=gen, device="cuda")[1:1 + n]
    r0 = (torch.randn(n + 4, generator=gen, device="cuda") * 2.0 ** -11)[1:1 + n]
    h = torch.empty(n + 8, dtype=wt, device="cuda")[1:1 + n]
    xc, rc = x.cpu(), r0.cpu()
    for m in (n, (8 << 20) + 4096 + 11):
        res = torch.empty(m + 4, device="cuda")[1:1 + m]
        res.copy_(r0[:m])
        red.compress_ef(h[:m], res, x[:m], m, F32, wd)
        want_w, want_r = host_ef(xc[:m], rc[:m], wt)
        assert torch.equal(h[:m].cpu().view(torch.int16), want_w.view(torch.int16)), m
        assert torch.equal(res.cpu().view(torch.int32), want_r.view(torch.int32)), m


def test_bad_arguments_raise_before_any_launch(red):
    wide = torch.zeros(1000, device="cuda")
    res = torch.zeros(1000, device="cuda")
    wire = torch.zeros(1000, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError):
        red.compress_ef(wire, res[:999], wide, 1000, F32, DType.FLOAT16)      # residual short
    with pytest.raises(ValueError):
        red.compress_ef(wire[:999], res, wide, 1000, F32, DType.FLOAT16)
    for dt, wd, code in [(DType.FLOAT64, DType.FLOAT16, reducer.EDTYPE),
                         (DType.BFLOAT16, DType.FLOAT16, reducer.EDTYPE),
                         (DType.FLOAT16, DType.BFLOAT16, reducer.EDTYPE),
                         (F32, F32, reducer.EDTYPE), (F32, DType.INT32, reducer.EDTYPE)]:
        with pytest.raises(reducer.ReduceError) as e:
            red.compress_ef(wire.data_ptr(), res.data_ptr(), wide.data_ptr(), 500, dt, wd)
        assert e.value.code == code
    for args in [(wire, wide, wide), (wire, res, res), (wire, res[4:], res[:-4]),
                 (wire, None, wide)]:
        with pytest.raises(reducer.ReduceError) as e:
            red.compress_ef(args[0], args[1], args[2], 996, F32, DType.BFLOAT16)
        assert e.value.code == reducer.EARGS
    red.compress_ef(None, None, None, 0, F32, DType.FLOAT16)                  # nothing to do
    torch.cuda.synchronize()
    assert float(wide.abs().sum()) == 0.0 and float(res.abs().sum()) == 0.0
    assert float(wire.float().abs().sum()) == 0.0


def test_torch_ops_opcheck_and_compression(red, data):
    from prophet_amd import torch_ops  # noqa: F401
    from prophet_amd.compression import Compression
    g, r = data
    n = 4099
    x, r0 = g[1000:1000 + n].cuda(), r[1000:1000 + n].cuda()
    utils = ("test_schema", "test_faketensor")
    for name, wt, comp in (("fp16", torch.float16, Compression.fp16_ef),
                           ("bf16", torch.bfloat16, Compression.bf16_ef)):
        op = getattr(torch.ops.bpsr, f"compress_{name}_ef_out")
        want_w, want_r = host_ef(x.cpu(), r0.cpu(), wt)
        dst, res = torch.empty(n, dtype=wt, device="cuda"), r0.clone()
        op(dst, res, x)                                         # mutates dst and resid
        assert _wire_mismatches(dst, want_w) == 0
        assert torch.equal(res.cpu().view(torch.int32), want_r.view(torch.int32))
        torch.library.opcheck(op.default, (torch.empty(n, dtype=wt, device="cuda"), r0.clone(), x),
                              test_utils=utils)
        # the Compression front end takes the same kernel for device tensors
        out, res2 = comp.wire_like(x), r0.clone()
        assert comp.compress_ef_into(out, res2, x) is out
        assert torch.equal(out.view(torch.int16), dst.view(torch.int16))
        assert torch.equal(res2.view(torch.int32), res.view(torch.int32))
        zero = comp.residual_like(x)
        assert zero.is_cuda and zero.dtype == torch.float32 and not bool(zero.any())
        with pytest.raises(Exception):
            op(dst, res.double(), x)                            # residual must be f32
        with pytest.raises(Exception):
            op(dst, res, x.double())                            # f32 only
        with pytest.raises(Exception):
            op(dst, res[:-1], x)
