"""Cast plans over the bf16 wire (byteps_reduce_cast_plan_create_wire,
prophet_amd/csrc/bpsr_k_cast_plan_bf16.hip) on the GPU: one launch over a
dozen segments against the one-tensor bf16 calls (bit for bit, sentinel bytes
between the segments intact) and against the host, a plan made by
create_wire(FLOAT16) against one made by create, a ``CastPlanCache`` asked for
an fp16 and a bf16 plan over the same addresses, and the 4-unit tile in a
child process started with BPSR_COPY_VPT=4: this file, run as a script."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from prophet_amd.compression import CastPlanCache  # noqa: E402
from prophet_amd.dtypes import DType, from_torch  # noqa: E402
from prophet_amd.reducer import CastDesc, GpuReducer  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

BF = DType.BFLOAT16
WIDE = [torch.float32, torch.float64, torch.float16]
IDS = ["f32", "f64", "f16"]
BITS = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32,
        torch.float64: torch.int64}
TILE = 256 * 8
SENTINEL = 0xA5
GAP = 64            # sentinel bytes between segments, at least


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return GpuReducer(device=0)


def _bits(t):
    return t.contiguous().view(BITS[t.dtype])


def _mismatches(got, want) -> int:
    got = got.cpu()
    nan = torch.isnan(want)
    bad = (_bits(got) != _bits(want)) & ~nan
    bad |= nan & ~torch.isnan(got)
    return int(bad.sum())


def _arena(nbytes):
    """A sentinel-filled device byte buffer whose first byte is 256-byte aligned."""
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    skip = (-raw.data_ptr()) % 256
    a = raw[skip:skip + nbytes]
    a.fill_(SENTINEL)
    return a


def _values(n):
    """f64 values whose first 32 hold what the bf16 casts must get right: f32
    overflow, f32-subnormal results and quotients, ties, signed zeros, a NaN."""
    rng = np.random.default_rng(31)
    x = rng.standard_normal(n) * np.exp2(rng.integers(-140, 127, n))
    special = [3.4028235677973366e38, 3.39e38, -3.4e38, 7e4, -65520.0, 1e-40, -1e-40, 2e-38,
               -3e-38, 0.0, -0.0, 1 + 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 3 * 2.0 ** -8,
               1 + 2.0 ** -8 + 2.0 ** -40, float("nan"), 3.0, 1 / 3, 2.0 ** -126, 2.0 ** -133]
    x[:len(special)] = special
    return x


# (elements, wide offset, bf16 offset), offsets in BYTES past a 256-byte
# boundary: an empty segment, less than a unit, one partial tile, exact and
# several full tiles, heads on both sides that co-align, a pair that never
# does, and element-misaligned operands.
def _layout(es):
    return [(0, 0, 0), (5, 0, 0), (9, es, 2), (TILE - 1, 0, 0), (TILE, 3 * es, 6),
            (TILE + 1, es, 2), (3 * TILE + 5, 0, 0), (3 * TILE + 5, 3 * es, 6),
            (2 * TILE + 77, 0, 2), (1, 0, 0), (TILE + 1, 1, 0), (9, 0, 1), (4 * TILE, 0, 0)]


class _Arenas:
    def __init__(self, dt, layout):
        self.es = es = torch.empty((), dtype=dt).element_size()
        self.layout = layout
        self.woff, self.hoff = [], []
        wc = hc = 256
        for n, wo, ho in layout:
            wc = (wc + 255) // 256 * 256
            hc = (hc + 255) // 256 * 256
            self.woff.append(wc + wo)
            self.hoff.append(hc + ho)
            wc += wo + n * es + GAP
            hc += ho + n * 2 + GAP
        self.wbytes, self.hbytes = wc + 256, hc + 256

    def mask(self, nbytes, offs, width):
        m = torch.zeros(nbytes, dtype=torch.bool)
        for (n, _, _), o in zip(self.layout, offs):
            m[o:o + n * width] = True
        return m


@pytest.mark.parametrize("dt", WIDE, ids=IDS)
def test_segments_against_the_one_tensor_calls_and_the_host(red, dt):
    lay = _Arenas(dt, _layout(torch.empty((), dtype=dt).element_size()))
    es, dtype = lay.es, from_torch(dt)
    nmax = max(n for n, _, _ in lay.layout)
    base = torch.from_numpy(_values(nmax + 64)).to(dt)
    base_bytes = base.view(torch.uint8).cuda()
    starts = [(5 * i) % 32 for i in range(len(lay.layout))]
    W, H = _arena(lay.wbytes), _arena(lay.hbytes)
    for (n, _, _), o, s in zip(lay.layout, lay.woff, starts):
        W[o:o + n * es] = base_bytes[s * es:(s + n) * es]
    W_in = W.clone()
    segs = [(W.data_ptr() + wo, H.data_ptr() + ho, n)
            for (n, _, _), wo, ho in zip(lay.layout, lay.woff, lay.hoff)]
    plan = red.cast_plan(segs, dtype, BF)
    assert plan.wire_dtype == BF
    cur = torch.cuda.current_stream()                      # raw pointers name no device
    plan.compress(stream=cur)
    H_one = _arena(lay.hbytes)
    for (n, _, _), wo, ho in zip(lay.layout, lay.woff, lay.hoff):
        red.compress(H_one.data_ptr() + ho, W.data_ptr() + wo, n, dtype, BF, stream=cur)
    assert torch.equal(H, H_one)
    assert torch.equal(W, W_in)
    Hc = H.cpu()
    assert bool((Hc[~lay.mask(lay.hbytes, lay.hoff, 2)] == SENTINEL).all())
    nans = 0
    for (n, _, _), ho, s in zip(lay.layout, lay.hoff, starts):
        want = base[s:s + n].to(torch.bfloat16)
        got = Hc[ho:ho + 2 * n].clone().view(torch.bfloat16)
        assert _mismatches(got, want) == 0, (n, ho)
        nans += int(torch.isnan(want).sum())
    assert nans >= 3                                       # the NaN is in several segments
    for divisor in (1, 3):
        W.fill_(SENTINEL)
        plan.decompress(divisor, stream=cur)
        W_one = _arena(lay.wbytes)
        for (n, _, _), wo, ho in zip(lay.layout, lay.woff, lay.hoff):
            red.decompress(W_one.data_ptr() + wo, H.data_ptr() + ho, n, dtype, BF, divisor,
                           stream=cur)
        assert torch.equal(W, W_one), divisor
        assert torch.equal(H, H_one)
        Wc = W.cpu()
        assert bool((Wc[~lay.mask(lay.wbytes, lay.woff, es)] == SENTINEL).all())
        for (n, _, _), wo, ho in zip(lay.layout, lay.woff, lay.hoff):
            # the host's input is what the device wrote (NaN payloads included)
            h = Hc[ho:ho + 2 * n].clone().view(torch.bfloat16)
            want = (h.clone().div_(divisor) if divisor > 1 else h).to(dt)
            got = Wc[wo:wo + n * es].clone().view(dt)
            assert _mismatches(got, want) == 0, (divisor, n, wo)
    plan.close()
    plan.close()                                           # idempotent


def test_create_wire_with_fp16_is_create(red):
    g = torch.Generator(device="cuda").manual_seed(5)
    sizes = [7, TILE + 1, 3 * TILE + 5]
    xs = [torch.randn(n + 8, generator=g, device="cuda")[i:i + n] * 3e4
          for i, n in enumerate(sizes)]
    ha = [torch.zeros(n + 8, dtype=torch.float16, device="cuda")[i:i + n]
          for i, n in enumerate(sizes)]
    hb = [torch.zeros_like(h) for h in ha]
    xb = [x.clone() for x in xs]
    plain = red.cast_plan([(x, h, x.numel()) for x, h in zip(xs, ha)], DType.FLOAT32)
    assert plain.wire_dtype == DType.FLOAT16
    # the same segments (other buffers) through the new entry point
    lib, stream = red.lib, int(torch.cuda.current_stream().cuda_stream)
    descs = (CastDesc * len(xb))()
    for i, (x, h) in enumerate(zip(xb, hb)):
        descs[i].wide, descs[i].half, descs[i].nelem = x.data_ptr(), h.data_ptr(), x.numel()
    wired = ctypes.c_void_p()
    assert lib.byteps_reduce_cast_plan_create_wire(descs, len(xb), int(DType.FLOAT32),
                                                   int(DType.FLOAT16), ctypes.byref(wired)) == 0
    plain.compress()
    assert lib.byteps_reduce_cast_plan_compress(wired, stream) == 0
    for a, b, x in zip(ha, hb, xs):
        assert torch.equal(_bits(a), _bits(b))
        assert torch.equal(_bits(a), _bits(x.to(torch.float16)))
    assert bool(torch.isinf(ha[2]).any())
    for x in xs + xb:
        x.fill_(-1.0)
    plain.decompress(3)
    assert lib.byteps_reduce_cast_plan_decompress(wired, 3, stream) == 0
    for x, y, h in zip(xs, xb, ha):
        one = torch.empty_like(x)
        red.decompress_fp16(one, h, x.numel(), DType.FLOAT32, 3)
        assert torch.equal(_bits(x), _bits(y)) and torch.equal(_bits(x), _bits(one))
    plain.close()
    assert lib.byteps_reduce_cast_plan_destroy(wired) == 0


def test_plan_cache_keeps_fp16_and_bf16_plans_apart(red):
    g = torch.Generator(device="cuda").manual_seed(6)
    x = torch.randn(TILE + 9, generator=g, device="cuda") * 3e4
    raw = torch.zeros(TILE + 9, dtype=torch.int16, device="cuda")   # one buffer, two readings
    cache = CastPlanCache(4)
    pf = cache.get(DType.FLOAT32, [(x, raw.view(torch.float16))], DType.FLOAT16)
    pb = cache.get(DType.FLOAT32, [(x, raw.view(torch.bfloat16))], DType.BFLOAT16)
    assert pf is not pb and cache.built == 2 and len(cache) == 2
    assert cache.get(DType.FLOAT32, [(x, raw.view(torch.float16))]) is pf      # default: fp16
    assert cache.get(DType.FLOAT32, [(x, raw.view(torch.bfloat16))], DType.BFLOAT16) is pb
    assert cache.built == 2
    pf.compress()
    assert torch.equal(raw, _bits(x.to(torch.float16)))
    pb.compress()
    assert torch.equal(raw, _bits(x.to(torch.bfloat16)))
    assert bool(torch.isfinite(raw.view(torch.bfloat16)).all())
    cache.close()
    assert len(cache) == 0


def _big_case(red, total, report=None):
    """One f32 plan of `total` elements and more over the bf16 wire: a few
    large segments at odd offsets plus small odd ones, compared on the device
    with the one-tensor bf16 kernels (which tests/test_compress_bf16_gpu.py
    pins to the host); a slice of each large segment also goes to the host."""
    g = torch.Generator(device="cuda").manual_seed(41)
    big = [total // 2 + 13, total // 4 + 4096 + 11, total // 4]
    small = [7, 4097, 1, 3 * TILE + 5]
    xs, hs = [], []
    for i, n in enumerate(big + small):
        k = i % 4               # both sides k elements in: they co-align after 0, 7, 6, 5
        x = torch.randn(n + 8, generator=g, device="cuda")
        x *= torch.exp2(torch.randint(-120, 120, (n + 8,), generator=g, device="cuda").float())
        xs.append(x[k:k + n])
        hs.append(torch.empty(n + 8, dtype=torch.bfloat16, device="cuda")[k:k + n])
    assert sum(big + small) >= total
    plan = red.cast_plan([(x, h, x.numel()) for x, h in zip(xs, hs)], DType.FLOAT32, BF)
    plan.compress()
    for x, h in zip(xs, hs):
        one = torch.empty_like(h)
        red.compress(one, x, x.numel(), DType.FLOAT32, BF)
        assert torch.equal(_bits(h), _bits(one))
    xin = [x.clone() for x in xs]
    for x in xs:
        x.fill_(-1.0)
    plan.decompress(3)
    for x, h, x0 in zip(xs, hs, xin):
        one = torch.empty_like(x)
        red.decompress(one, h, x.numel(), DType.FLOAT32, BF, 3)
        assert torch.equal(_bits(x), _bits(one))
        m = min(x.numel(), 100_000)
        hw = x0[-m:].cpu().to(torch.bfloat16)
        assert torch.equal(_bits(h[-m:].cpu()), _bits(hw))
        assert torch.equal(_bits(x[-m:].cpu()), _bits(hw.div_(3).float()))
    plan.close()
    if report:
        print(report)


def test_four_unit_tiles_in_a_child_process():
    """BPSR_COPY_VPT=4 and 32 Mi elements (4096 tiles of 4 units): the plan is
    cut for 4 units per lane, with non-temporal stores one way.  A fresh child
    process: the library reads its tuning once."""
    env = dict(os.environ, BPSR_COPY_VPT="4")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "four-unit bf16 case passed" in r.stdout


if __name__ == "__main__":
    _big_case(GpuReducer(device=0), 32 << 20, report="four-unit bf16 case passed")
