"""The stochastic-rounding compress kernels (the scheme of
prophet_amd/csrc/bpsr_cast_sr.h over bpsr_cast_impl.h and bpsr_cast_single.h;
bpsr_k_cast_sr.hip, bpsr_k_cast_sr_bf16.hip) on the GPU against the host
definition (prophet_amd/sr.py): the wire bits are equal everywhere except
where the expected value is a NaN (there only a NaN is required: the payload
is not part of the contract)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from prophet_amd import reducer, sr  # noqa: E402
from prophet_amd.dtypes import DType  # noqa: E402
from prophet_amd.reducer import GpuReducer  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

F32 = DType.FLOAT32
WIRES = [(DType.FLOAT16, torch.float16, "fp16"), (DType.BFLOAT16, torch.bfloat16, "bf16")]
IDS = ["fp16", "bf16"]
# Launches this short run tiles of 256 lanes x 8 elements x 1 unit per lane
TILE = 256 * 8
KEYS = (0x1234, 0xfedcba98)
STEPS = (0, 1, 0xffffffff)


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return GpuReducer(device=0)


def _specials():
    """The g list of tests/test_compress_ef_gpu.py:_specials."""
    g = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00008000, 0x00008001,
         0x00800000,
         0x3f800fff, 0x3f801000, 0x3f801001, 0x3f802fff, 0x3f803000, 0x3f803001,
         0x33000000, 0x33000001, 0x33800000, 0x33c00000, 0x32ffffff,
         0x3f807fff, 0x3f808000, 0x3f808001, 0x3f817fff, 0x3f818000, 0x3f818001,
         0x477fdfff, 0x477fe000, 0xc77fdfff, 0xc77fe000, 0x7f7f7fff, 0x7f7f8000, 0xff7f8000,
         0x7f7fffff, 0xff7fffff,
         0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001]
    return np.asarray(g, np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def data():
    """1 << 18 f32 values spread over the decades with the specials repeated
    at the front, so that each special meets many different draws.  Computed
    once, shared, left unchanged."""
    rng = np.random.default_rng(41)
    n = 1 << 18
    with np.errstate(over="ignore"):
        g = (rng.standard_normal(n) * np.exp2(rng.uniform(-140.0, 127.0, n))).astype(np.float32)
    sp = np.tile(_specials(), 64)
    g[:sp.size] = sp
    return g


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _mismatches(got_bits, want_bits, g, name) -> int:
    """Wire words that differ, NaN positions excepted (a NaN is required)."""
    nan = np.isnan(g)
    bad = (got_bits != want_bits) & ~nan
    if name == "bf16":
        got_nan = ((got_bits & 0x7f80) == 0x7f80) & ((got_bits & 0x7f) != 0)
    else:
        got_nan = ((got_bits & 0x7c00) == 0x7c00) & ((got_bits & 0x3ff) != 0)
    return int(bad.sum() + (nan & ~got_nan).sum())


@pytest.mark.parametrize("wd,wt,name", WIRES, ids=IDS)
def test_bits_match_the_host_definition(red, data, wd, wt, name):
    n = data.size
    gd = torch.from_numpy(data).cuda()
    out = torch.empty(n, dtype=wt, device="cuda")
    seen = []
    for key in KEYS:
        for step in STEPS:
            red.compress_sr(out, gd, n, key, step, wd)
            got = _bits(out)
            want = sr.sr_round(data, key, step, name)
            assert _mismatches(got, want, data, name) == 0, (hex(key), hex(step))
            seen.append(got)
    # the same (key, step) twice: the same bytes; another step or key: other bytes
    red.compress_sr(out, gd, n, KEYS[-1], STEPS[-1], wd)
    assert np.array_equal(_bits(out), seen[-1])
    for a in range(len(seen)):
        for b in range(a + 1, len(seen)):
            assert not np.array_equal(seen[a], seen[b])
    assert torch.equal(gd.cpu().view(torch.int32), torch.from_numpy(data).view(torch.int32))
    # inf and NaN are the plain compress's; a value the wire holds is sent unchanged
    plain = torch.empty_like(out)
    red.compress(plain, gd, n, F32, wd)
    pb = _bits(plain)
    back = plain.float().cpu().numpy()
    keep = (~np.isfinite(data) | (back == data)) & ~np.isnan(data)
    assert keep.sum() > 100 and np.array_equal(seen[0][keep], pb[keep])
    # both neighbours occur: the draw matters
    assert (seen[0] != pb).any()


SIZES = (1, 3, 4, 5, TILE - 1, TILE, TILE + 9, 3 * 8192 + 13)
WIDE_OFFS = (0, 1, 2, 3)    # elements from a 16-byte boundary
WIRE_OFFS = (0, 1, 2, 3)   # elements; the sides co-align iff the offsets agree
GUARD = 64                  # bytes


def _aligned_bytes(nbytes):
    """A device byte buffer whose first byte is 256-byte aligned."""
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    skip = (-raw.data_ptr()) % 256
    return raw[skip:skip + nbytes]


@pytest.mark.parametrize("wd,wt,name", WIRES, ids=IDS)
def test_geometry_offsets_tails_and_guards(red, data, wd, wt, name):
    """Every length around the 4-element Philox group, the 8-element unit and
    the tile; the wide base 0-3 elements past a 16-byte boundary (where the
    cut's head is no multiple of 4 and a vector straddles two groups, or where
    the two sides never co-align and every element takes the element path),
    the wire base 0-3.  The element index, not the address, picks the
    bits: one expected array serves every offset.  0xA5 guard bytes around
    dst stay intact."""
    nmax = max(SIZES)
    g = data[4000:4000 + nmax]                  # past the specials: no NaN
    key, step = 0xabcdef01, 3
    want = torch.from_numpy(sr.sr_round(g, key, step, name).view(np.int16)).cuda()
    sbuf = _aligned_bytes((nmax + 4) * 4)
    dbuf = _aligned_bytes(256 + (nmax + 8) * 2 + GUARD)
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    gd = torch.from_numpy(g).cuda()
    for so in WIDE_OFFS:
        src = sbuf[so * 4:(so + nmax) * 4].view(torch.float32)
        src.copy_(gd)
        for do in WIRE_OFFS:
            d0 = 256 + do * 2
            for n in SIZES:
                dbuf.fill_(0xA5)
                dst = dbuf[d0:d0 + n * 2].view(wt)
                red.compress_sr(dst, src, n, key, step, wd)
                bad += (dst.view(torch.int16) != want[:n]).sum()
                bad += (dbuf[d0 - GUARD:d0] != 0xA5).sum()
                bad += (dbuf[d0 + n * 2:d0 + n * 2 + GUARD] != 0xA5).sum()
    assert not np.isnan(g).any()
    assert int(bad) == 0


def _big_case(red, units):
    """2048 full tiles of `units` units a lane, a partial tile, a head of 7
    (wide base one element past a 16-byte boundary: every vector straddles two
    Philox groups) and a tail, both wires under one set of draws."""
    n = 2048 * units * TILE + TILE + 7 + 5
    rng = np.random.default_rng(43)
    g = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 20, n))).astype(np.float32)
    r16 = sr.sr_bits(n, 77, 5)
    gd = torch.empty(n + 8, device="cuda")[1:1 + n]
    gd.copy_(torch.from_numpy(g))
    for wd, wt, name in WIRES:
        out = torch.empty(n + 16, dtype=wt, device="cuda")[1:1 + n]
        red.compress_sr(out, gd, n, 77, 5, wd)
        want = (sr.sr_bf16 if name == "bf16" else sr.sr_fp16)(g, r16)
        assert np.array_equal(_bits(out), want), (units, name)


def test_two_unit_tiles(red):
    """The launch keeps copy_vpt's 2 units a lane from 2048 such tiles on
    (8 Mi elements); every shorter launch in this file runs 1 unit a lane."""
    _big_case(red, 2)


def test_four_unit_tiles_in_a_child_process():
    """copy_vpt = 4 is read from BPSR_COPY_VPT once a process: this file, run
    as a script with it set, runs 2048 tiles of 4 units a lane."""
    env = dict(os.environ, BPSR_COPY_VPT="4")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "four-unit case passed" in r.stdout


def test_one_byte_misaligned_operands(red, data):
    """An operand one byte past its element alignment: every element through
    the byte-wise element path."""
    n = TILE + 9
    g = data[5000:5000 + n]
    want = sr.sr_round(g, 9, 9, "fp16").view(np.uint8)
    for which in ("src", "dst"):
        so, do = (1 if which == "src" else 0), 128 + (1 if which == "dst" else 0)
        sbuf = _aligned_bytes(n * 4 + 16)
        dbuf = _aligned_bytes(256 + n * 2 + 256)
        dbuf.fill_(0xA5)
        sbuf[so:so + n * 4].copy_(torch.from_numpy(g.view(np.uint8)).cuda())
        red.compress_sr(dbuf.data_ptr() + do, sbuf.data_ptr() + so, n, 9, 9, DType.FLOAT16,
                        stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert np.array_equal(dbuf[do:do + n * 2].cpu().numpy(), want), which
        assert bool((dbuf[:do] == 0xA5).all()) and bool((dbuf[do + n * 2:] == 0xA5).all())


def test_bad_arguments_raise_before_any_launch(red):
    wide = torch.zeros(1000, device="cuda")
    wire = torch.zeros(1000, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError):
        red.compress_sr(wire[:999], wide, 1000, 1, 2, DType.FLOAT16)
    for dt, wd in [(DType.FLOAT64, DType.FLOAT16), (DType.BFLOAT16, DType.FLOAT16),
                   (DType.FLOAT16, DType.BFLOAT16), (F32, F32), (F32, DType.INT32)]:
        with pytest.raises(reducer.ReduceError) as e:
            red.compress_sr(wire.data_ptr(), wide.data_ptr(), 500, 1, 2, wd, src_dtype=dt)
        assert e.value.code == reducer.EDTYPE
    for args in [(wide.view(torch.float16)[:1000], wide), (wire, None), (None, wide)]:
        with pytest.raises(reducer.ReduceError) as e:
            red.compress_sr(args[0], args[1], 1000, 1, 2, DType.FLOAT16)
        assert e.value.code == reducer.EARGS
    red.compress_sr(None, None, 0, 1, 2, DType.FLOAT16)                      # nothing to do
    torch.cuda.synchronize()
    assert float(wide.abs().sum()) == 0.0 and float(wire.float().abs().sum()) == 0.0


def test_torch_ops_on_a_side_stream_and_compression(red, data):
    """The two ops run on the current stream of a non-default stream (ordered
    behind the work that produced their input there), pass opcheck, and are
    what the Compression front end launches for device tensors."""
    from prophet_amd import torch_ops  # noqa: F401
    from prophet_amd.compression import Compression
    n = 4099
    g = data[2000:2000 + n]
    utils = ("test_schema", "test_faketensor")
    side = torch.cuda.Stream()
    for name, wt, comp in (("fp16", torch.float16, Compression.fp16_sr),
                           ("bf16", torch.bfloat16, Compression.bf16_sr)):
        op = getattr(torch.ops.bpsr, f"compress_{name}_sr_out")
        want = sr.sr_round(g, 0x55, 8, name)
        half = torch.from_numpy(g * np.float32(0.5)).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            x = half * 2                                      # produced on the side stream
            dst = torch.empty(n, dtype=wt, device="cuda")
            op(dst, x, 0x55, 8)
        side.synchronize()
        assert _mismatches(_bits(dst), want, g, name) == 0
        torch.library.opcheck(op.default, (torch.empty(n, dtype=wt, device="cuda"), x, 0x55, 8),
                              test_utils=utils)
        out = comp.wire_like(x)
        assert comp.compress_sr_into(out, x, 0x55, 8) is out
        assert np.array_equal(_bits(out), _bits(dst))
        with pytest.raises(Exception):
            op(dst, x.double(), 1, 2)                           # f32 only
        with pytest.raises(Exception):
            op(dst[:-1], x, 1, 2)
        with pytest.raises(Exception):
            op(dst.float(), x, 1, 2)                            # dst of the wire dtype


if __name__ == "__main__":
    assert os.environ.get("BPSR_COPY_VPT") == "4"
    _big_case(GpuReducer(device=0), 4)
    print("four-unit case passed")
