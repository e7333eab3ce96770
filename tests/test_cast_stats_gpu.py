"""The decompress with statistics (byteps_reduce_cast_plan_decompress_stats,
the STATS variant of cast_plan_kernel plus the finish kernel)
on the GPU, both wires, the three wide dtypes of each, divisors 1 and 8.

Per plan: the bytes written — the whole buffers, the sentinel bytes around
every segment included — equal the plain decompress's; every row of a
NaN-prefilled ``stats`` is overwritten; a second launch gives the same bits
with no reset in between; and the rows equal the pinned definition
(``compression.decompress_stats``'s numpy lines) applied to the bytes written.
Where the wire values are small integers times powers of two every partial sum
is exact in f64, so the sum of squares must match BIT FOR BIT whatever the
order; random values must match within ``nelem * 2**-52 * ref``, the
first-order bound of an any-order f64 sum of non-negative terms with one
rounding each.

The tile size comes from the library's tuning, which a process reads once, so
the 4-unit shape runs in a child process started with BPSR_COPY_VPT=4: this
file, run as a script (as tests/test_cast_plan_gpu.py does)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from prophet_amd import reducer  # noqa: E402
from prophet_amd.dtypes import from_torch  # noqa: E402
from prophet_amd.reducer import GpuReducer, SrKey  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

_HDR = open(os.path.join(ROOT, "prophet_amd", "csrc", "bpsr_internal.h")).read()
K_BLOCK = int(re.search(r"constexpr int kBlock = (\d+);", _HDR).group(1))
K_MIN_TILES = int(re.search(r"constexpr uint64_t kMinTiles = (\d+);", _HDR).group(1))
ELEM_PART = K_BLOCK * 16                 # kCastElemPart: elements of one element record
TILE = K_BLOCK * 8                       # elements of a 1-unit tile (every small plan)
SENTINEL = 0xA5
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
PAIRS = [(F16, F32), (F16, F64), (F16, BF16), (BF16, F32), (BF16, F64), (BF16, F16)]
PAIR_IDS = ["fp16-f32", "fp16-f64", "fp16-bf16", "bf16-f32", "bf16-f64", "bf16-fp16"]
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return GpuReducer(device=0)


def _es(dt):
    return torch.empty((), dtype=dt).element_size()


def _offsets(k, es):
    """Byte offsets past a 16-byte boundary of the wide and the 2-byte operand
    whose vectors first co-align after k elements (cast_cut: the 2-byte side
    aligns every 8 elements, the wide side every 16 / es)."""
    return (16 - es * (k % (16 // es))) % 16, (16 - 2 * k) % 16


def _exact(n, wire, seed):
    """n wire values on the device, small integers times powers of two: every
    square, and every partial sum of squares of up to 2^24 of them, is exact
    in f64, also after a divide by 8 and in either 2-byte wide type."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    m = torch.randint(-8, 9, (n,), generator=g, device="cuda").float()
    e = torch.randint(-2, 4, (n,), generator=g, device="cuda").float()
    return (m * torch.exp2(e)).to(wire)


def _put(x, where):
    """x with ``where``: {index: value} written in (indices past the end are
    skipped, negative ones count from the end)."""
    n = x.numel()
    for i, v in where.items():
        if -n <= i < n:
            x[i] = v
    return x


class _Seg:
    """One segment: its wire values in a sentinel-filled buffer of each side,
    the operands ``woff`` / ``hoff`` bytes past a 256-byte boundary."""

    def __init__(self, values, wide, woff=0, hoff=0, resid=False):
        self.n, self.wide, self.es = values.numel(), wide, _es(wide)
        self.W, self.wptr = self._buf(self.n * self.es, woff)
        self.H, self.hptr = self._buf(self.n * 2, hoff)
        self.woff, self.hoff = self.wptr - self.W.data_ptr(), self.hptr - self.H.data_ptr()
        self.H[self.hoff:self.hoff + 2 * self.n] = values.contiguous().view(torch.uint8)
        if resid:                             # f32 beside the wide operand, co-aligned
            self.R, self.rptr = self._buf(self.n * 4, woff)

    @staticmethod
    def _buf(nbytes, off):
        raw = torch.full((nbytes + 768,), SENTINEL, dtype=torch.uint8, device="cuda")
        start = raw.data_ptr() + (-raw.data_ptr()) % 256 + 256 + off
        return raw, start

    def written(self):
        """What the decompress wrote, on the host, as the wide dtype."""
        b = self.W[self.woff:self.woff + self.n * self.es].clone()
        return b.view(self.wide).cpu()


def _definition(out):
    x = out.to(torch.float64).numpy().reshape(-1)
    fin = np.isfinite(x)
    return float(np.square(x[fin]).sum()), int(np.count_nonzero(~fin))


def _plan(red, segs, wire, kind):
    wide = segs[0].wide
    if kind == "ef":
        desc = [(s.wptr, s.hptr, s.n, s.rptr) for s in segs]
    elif kind == "sr":
        desc = [(s.wptr, s.hptr, s.n, SrKey(17 + i)) for i, s in enumerate(segs)]
    else:
        desc = [(s.wptr, s.hptr, s.n) for s in segs]
    return red.cast_plan(desc, from_torch(wide), from_torch(wire))


def _check(red, segs, wire, divisor, kind="plain", exact=True, report=None):
    """The whole contract of one plan; returns the rows and the references."""
    cur = torch.cuda.current_stream()             # raw pointers name no device
    plan = _plan(red, segs, wire, kind)
    plan.decompress(divisor, stream=cur)
    plain = [s.W.clone() for s in segs]
    halves = [s.H.clone() for s in segs]
    rows = []
    for launch in range(2):                       # a relaunch needs no reset
        for s in segs:
            s.W.fill_(SENTINEL)
        st = torch.full((2 * len(segs),), NAN, dtype=F64, device="cuda")
        plan.decompress(divisor, stream=cur, stats=st)
        for s, p, h in zip(segs, plain, halves):
            assert torch.equal(s.W, p), "the bytes are the plain decompress's"
            assert torch.equal(s.H, h)
        rows.append(st.cpu())
    assert not bool(torch.isnan(rows[0]).any()), "every row is overwritten"
    assert torch.equal(rows[0].view(torch.int64), rows[1].view(torch.int64)), "same bits twice"
    got = rows[0].view(-1, 2)
    refs = []
    for i, s in enumerate(segs):
        ss, nf = _definition(s.written())
        refs.append((ss, nf))
        print(f"{report or ''} seg {i} n={s.n}: sumsq {float(got[i, 0])!r} ref {ss!r} "
              f"nonfinite {float(got[i, 1])} ref {nf}")
        assert float(got[i, 1]) == nf, (i, s.n)
        if exact:
            assert float(got[i, 0]) == ss, (i, s.n)
        else:
            assert abs(float(got[i, 0]) - ss) <= s.n * 2.0 ** -52 * ss, (i, s.n)
    plan.close()
    return got, refs


# ------------------------------------------------------------------ sizes --
SIZES = (0, 1, 7, 8, 9, TILE - 1, TILE, TILE + 1, TILE + 3 * 8 + 5)


@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("wire,wide", PAIRS, ids=PAIR_IDS)
def test_sizes_exact(red, wire, wide, divisor):
    segs = [_Seg(_exact(n, wire, 100 + n), wide) for n in SIZES]
    got, refs = _check(red, segs, wire, divisor)
    assert got[0].tolist() == [0.0, 0.0]                     # nelem == 0
    assert all(nf == 0 for _, nf in refs) and sum(ss for ss, _ in refs) > 0


@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("wire,wide", PAIRS, ids=PAIR_IDS)
def test_heads_element_records_and_a_mixed_plan(red, wire, wide, divisor):
    es = _es(wide)
    k = 3
    wo, ho = _offsets(k, es)
    never = 2 * ELEM_PART + 5                                # three element records
    segs = [
        _Seg(_exact(k + 2 * TILE + 3 * 8 + 5, wire, 1), wide, wo, ho),   # head, tiles, tail
        _Seg(_exact(never, wire, 2), wide, 0, 2),            # never co-aligns
        _Seg(_exact(0, wire, 3), wide),                      # empty, in the middle
        _Seg(_exact(TILE + 1, wire, 4), wide, *_offsets(5, es)),
        _Seg(_exact(9, wire, 5), wide),
    ]
    got, refs = _check(red, segs, wire, divisor)
    assert got[2].tolist() == [0.0, 0.0]


# --------------------------------------------------------- non-finite values --
def _paths(wire, wide, fill=None, seed=50):
    """One segment per path — full tile, guarded partial tile, element range,
    and all of them behind a head — filled with ``fill`` or exact values."""
    k = 3
    wo, ho = _offsets(k, _es(wide))
    out = []
    for i, (n, w, h) in enumerate([(TILE, 0, 0), (1000, 0, 0), (7, 0, 0), (300, 0, 2),
                                   (k + 2 * TILE + 3 * 8 + 5, wo, ho)]):
        v = _exact(n, wire, seed + i)
        if fill is not None:
            v.fill_(fill)
        out.append(_Seg(v, wide, w, h))
    return out


@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("wire,wide", PAIRS, ids=PAIR_IDS)
def test_all_nan_segments_count_every_element_once(red, wire, wide, divisor):
    segs = _paths(wire, wide, fill=NAN)
    got, _ = _check(red, segs, wire, divisor)
    for i, s in enumerate(segs):
        assert got[i].tolist() == [0.0, float(s.n)]


@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("wire,wide", PAIRS, ids=PAIR_IDS)
def test_non_finite_values_at_the_edges(red, wire, wide, divisor):
    k = 3
    wo, ho = _offsets(k, _es(wide))
    n = k + 2 * TILE + 3 * 8 + 5
    last_tile = k + TILE
    where = {
        0: INF, n - 1: NAN,                                   # first / last; head and tail
        k - 1: -INF, k + 2 * TILE + 3 * 8 + 2: -INF,          # head's last, inside the tail
        k: NAN, k + 7: INF,                                   # first full tile, lane 0
        k + 255 * 8: -INF, k + 255 * 8 + 7: NAN,              # ... lane 255
        last_tile: INF, last_tile + 4: NAN,                   # last full tile, lane 0
        last_tile + 255 * 8 + 7: -INF,                        # ... lane 255
        k + 2 * TILE: NAN, k + 2 * TILE + 8 + 3: INF, k + 2 * TILE + 23: -INF,   # partial tile
    }
    segs = [_Seg(_put(_exact(n, wire, 7), where), wide, wo, ho)]
    for m in (1, 7, 8, 9, TILE, TILE + 1):                   # first and last of every shape
        segs.append(_Seg(_put(_exact(m, wire, 70 + m), {0: -INF, -1: NAN}), wide))
    got, refs = _check(red, segs, wire, divisor)
    assert refs[0][1] == len(where) == float(got[0, 1])
    assert [nf for _, nf in refs[1:]] == [1, 2, 2, 2, 2, 2]
    assert all(np.isfinite(float(got[i, 0])) for i in range(len(segs)))   # they are left out


def test_overflow_before_and_after_the_divide(red):
    """fp16 wire: 60000 is finite with and without the divide, inf never is.
    bf16 wire into fp16: 1e5 overflows the wide type (inf is written) unless
    the divide by 8 brings it into range first."""
    v = torch.tensor([60000.0, INF, 2.0, 65504.0], dtype=F16, device="cuda")
    for divisor, want in ((1, [60000.0 ** 2 + 4.0 + 65504.0 ** 2, 1.0]),
                          (8, [7500.0 ** 2 + 0.0625 + 8188.0 ** 2, 1.0])):
        got, _ = _check(red, [_Seg(v.clone(), F32)], F16, divisor)
        assert got[0].tolist() == want
    v = torch.tensor([99840.0, 2.0, -99840.0], dtype=BF16, device="cuda")   # 390 * 2^8
    got, _ = _check(red, [_Seg(v.clone(), F16)], BF16, 1)
    assert got[0].tolist() == [4.0, 2.0]
    got, _ = _check(red, [_Seg(v.clone(), F16)], BF16, 8)
    assert got[0].tolist() == [2 * 12480.0 ** 2 + 0.0625, 0.0]


# ------------------------------------------------------------ random values --
@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("wire,wide", PAIRS, ids=PAIR_IDS)
def test_random_values_within_the_any_order_bound(red, wire, wide, divisor):
    g = torch.Generator(device="cuda").manual_seed(9)
    segs = []
    for n, (wo, ho) in ((5 * TILE + 77, _offsets(3, _es(wide))), (1000, (0, 0)),
                        (ELEM_PART + 9, (0, 2))):
        x = torch.randn(n, generator=g, device="cuda")
        x *= torch.exp2(torch.randint(-12, 12, (n,), generator=g, device="cuda").float())
        segs.append(_Seg(_put(x.to(wire), {5: INF, n // 2: NAN}), wide, wo, ho))
    _check(red, segs, wire, divisor, exact=False)


# --------------------------------------------------- EF and SR plans, errors --
@pytest.mark.parametrize("kind", ["ef", "sr"])
@pytest.mark.parametrize("wire", [F16, BF16], ids=["fp16", "bf16"])
def test_error_feedback_and_stochastic_plans(red, wire, kind):
    for divisor in (1, 8):
        k = 3
        wo, ho = _offsets(k, 4)
        n = k + 2 * TILE + 3 * 8 + 5
        specs = [(_put(_exact(n, wire, 21), {0: INF, k: NAN, n - 1: -INF}), wo, ho),
                 (_exact(0, wire, 22), 0, 0), (_exact(1000, wire, 23), 0, 0),
                 (_exact(ELEM_PART + 5, wire, 24), 0, 2), (_exact(7, wire, 25).fill_(NAN), 0, 0)]
        segs = [_Seg(v, F32, w, h, resid=(kind == "ef")) for v, w, h in specs]
        resid = [s.R.clone() for s in segs] if kind == "ef" else []
        got, refs = _check(red, segs, wire, divisor, kind=kind)
        assert refs[0][1] == 3 and refs[4] == (0.0, 7) and got[1].tolist() == [0.0, 0.0]
        for s, r in zip(segs, resid):
            assert torch.equal(s.R, r)                        # the residuals are not touched


def test_bad_stats_raise_before_any_launch(red):
    cur = torch.cuda.current_stream()
    segs = [_Seg(_exact(TILE + 9, F16, 31), F64), _Seg(_exact(100, F16, 32), F64)]
    plan = _plan(red, segs, F16, "plain")
    before = [s.W.clone() for s in segs]
    ok = torch.zeros(4, dtype=F64, device="cuda")

    def refused(stats, divisor=1, exc=reducer.ReduceError):
        with pytest.raises(exc) as e:
            plan.decompress(divisor, stream=cur, stats=stats)
        if exc is reducer.ReduceError:
            assert e.value.code == reducer.EARGS

    s0 = segs[0]
    inside = s0.W[s0.woff:s0.woff + 32].view(F64)            # the first bytes of a wide range
    refused(inside)
    refused(s0.wptr + s0.n * 8 - 8)                          # raw pointer: its last 8 bytes
    refused(s0.wptr - 24)                                    # reaches 8 bytes into it
    refused(segs[1].hptr)                                    # a 2-byte side
    refused(ok.data_ptr() + 4)                               # not 8-byte aligned
    refused(0)                                               # null
    refused(ok, divisor=0)
    refused(torch.zeros(4, device="cuda"), exc=ValueError)                 # dtype
    refused(torch.zeros(6, dtype=F64, device="cuda"), exc=ValueError)      # size
    refused(torch.zeros(8, dtype=F64, device="cuda")[::2], exc=ValueError)  # not contiguous
    refused(torch.zeros(4, dtype=F64), exc=ValueError)                     # on the host
    torch.cuda.synchronize()
    for s, b in zip(segs, before):
        assert torch.equal(s.W, b)                           # nothing ran
    assert ok.tolist() == [0.0] * 4
    # touching ranges are fine: the 32 bytes right in front of a wide range
    front = s0.W[s0.woff - 32:s0.woff].view(F64)
    plan.decompress(1, stream=cur, stats=front)
    torch.cuda.synchronize()
    assert [float(front[1]), float(front[3])] == [0.0, 0.0] and float(front[0]) > 0
    plan.close()
    # a plan of no segments writes nothing and succeeds; one of only empty
    # segments writes its rows
    empty = red.cast_plan([], from_torch(F32))
    empty.decompress(1, stream=cur, stats=torch.empty(0, dtype=F64, device="cuda"))
    empty.close()
    st = torch.full((4,), NAN, dtype=F64, device="cuda")
    hollow = red.cast_plan([(0, 0, 0), (0, 0, 0)], from_torch(F32))
    hollow.decompress(3, stream=cur, stats=st)
    torch.cuda.synchronize()
    assert st.tolist() == [0.0] * 4
    hollow.close()


def test_compressors_and_plan_cache_on_the_device():
    """decompress_into / decompress_many_into with device tensors: one-segment
    and several-plan calls, the rows scattered into the caller's order."""
    from prophet_amd.compression import CastPlanCache, Compression
    comp = Compression.fp16
    outs = [torch.empty(300, device="cuda"), torch.empty(TILE + 9, dtype=F64, device="cuda"),
            torch.empty(0, device="cuda"), torch.empty(77, dtype=F64, device="cuda"),
            torch.empty(2 * TILE, device="cuda")]
    ws = [_put(_exact(o.numel(), F16, 40 + i), {1: INF}) for i, o in enumerate(outs)]
    cache = CastPlanCache(4)
    for _ in range(2):
        st = torch.full((len(outs), 2), NAN, dtype=F64, device="cuda")
        comp.decompress_many_into(outs, ws, 8, plans=cache, stats=st)
        for i, o in enumerate(outs):
            plain = torch.empty_like(o)
            comp.decompress_into(plain, ws[i], 8)
            assert torch.equal(o.view(torch.uint8), plain.view(torch.uint8))
            ss, nf = _definition(o.cpu())
            assert st[i].tolist() == [ss, float(nf)], i
    assert cache.built == 2                                   # f32 and f64: two plans, reused
    one = torch.full((2,), NAN, dtype=F64, device="cuda")
    comp.decompress_into(outs[1], ws[1], 1, stats=one)        # builds and destroys its plan
    assert one.tolist() == list(map(float, _definition(outs[1].cpu())))
    with pytest.raises(ValueError):
        comp.decompress_into(outs[1], ws[1], 1, stats=torch.empty(2, dtype=F64))
    cache.close()


# -------------------------------------------------------- larger tile sizes --
def _tile_case(red, u, wire, report=None):
    """One f32 plan just over the size where the tile-size rule picks u units
    a lane (kMinTiles tiles of kBlock * u units, with the library's copy tile
    at u or above), a head, a partial tile and a tail behind it, a small
    segment beside it."""
    k = 3
    n = k + (K_MIN_TILES + 1) * u * TILE + 3 * 8 + 5
    where = {0: INF, k: NAN, k + u * TILE - 1: -INF, n - 1: NAN,
             k + K_MIN_TILES * u * TILE: INF, k + (K_MIN_TILES + 1) * u * TILE + 9: -INF}
    wo, ho = _offsets(k, 4)
    segs = [_Seg(_put(_exact(n, wire, 60 + u), where), F32, wo, ho),
            _Seg(_exact(1000, wire, 61), F32)]
    got, refs = _check(red, segs, wire, 8, report=report)
    assert refs[0][1] == len(where)
    # u is not visible from here: a plan cut for fewer units would still pass.
    # The rule itself is pinned by tests/cpp/cast_table_stats.cpp ("u=2", "u=4").


@pytest.mark.parametrize("wire", [F16, BF16], ids=["fp16", "bf16"])
def test_two_unit_tiles(red, wire):
    _tile_case(red, 2, wire)


def test_four_unit_tiles_in_a_child_process():
    env = dict(os.environ, BPSR_COPY_VPT="4")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "four-unit case passed" in r.stdout


if __name__ == "__main__":
    _red = GpuReducer(device=0)
    for _wire in (F16, BF16):
        _tile_case(_red, 4, _wire)
    print("four-unit case passed")
