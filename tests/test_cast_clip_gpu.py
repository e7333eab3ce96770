"""Clip by global norm and unscale inside the decompress on
the GPU: byteps_reduce_cast_plan_measure (the MEASURE variant of
cast_plan_kernel plus the finish kernel), byteps_reduce_clip_record and
byteps_reduce_cast_plan_decompress_scaled (the SCALED variant), both wires,
the three wide dtypes of each, divisors 1 and 8, plain, error-feedback and
stochastic-rounding plans.

Measure: the rows equal the rows of ``decompress(stats=)`` on the same plan and
bytes BIT FOR BIT, every byte of the sentinel-filled wide buffers is unchanged,
a second launch gives the same bits with no reset, NaN-prefilled rows are all
overwritten.

Record, against ``compression.clip_record`` on the device's own rows:
``nonfinite`` exact; ``sumsq`` exact where every partial sum is exact (small
integers times powers of two), within ``nrows * 2**-52`` relative otherwise
(an any-order f64 sum of non-negative terms, one rounding each); ``norm``
within ``4 * 2**-52`` relative of ``sqrt(sumsq) * inv`` evaluated on the
device's ``sumsq`` (a sqrt that is correctly rounded or nearly so, and one
multiply); ``coef`` and ``mult`` within one f32 ulp of the definition's (an
f64 error of a few ``2**-52`` moves an f32 rounding by at most one step).

Scaled decompress: the bytes written equal torch's CPU arithmetic on the plain
decompress's output — ``* m`` in f32, then the cast to the wide dtype, or the
f64 product — with the ``mult`` read back from the device, bit for bit (NaN
positions as NaN-ness); the sentinel bytes around every segment are intact.

The tile size comes from the library's tuning, which a process reads once, so
the 2- and 4-unit shapes run in child processes started with BPSR_COPY_VPT:
this file, run as a script (as tests/test_cast_stats_gpu.py does)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from prophet_amd import compression, reducer  # noqa: E402
from prophet_amd.dtypes import from_torch  # noqa: E402
from prophet_amd.reducer import GpuReducer, SrKey  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

_HDR = open(os.path.join(ROOT, "prophet_amd", "csrc", "bpsr_internal.h")).read()
K_BLOCK = int(re.search(r"constexpr int kBlock = (\d+);", _HDR).group(1))
K_MIN_TILES = int(re.search(r"constexpr uint64_t kMinTiles = (\d+);", _HDR).group(1))
TILE = K_BLOCK * 8                       # elements of a 1-unit tile (every small plan)
SENTINEL = 0xA5
F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
PAIRS = [(F16, F32), (F16, F64), (F16, BF16), (BF16, F32), (BF16, F64), (BF16, F16)]
PAIR_IDS = ["fp16-f32", "fp16-f64", "fp16-bf16", "bf16-f32", "bf16-f64", "bf16-fp16"]
INF, NAN = float("inf"), float("nan")
EPS52 = 2.0 ** -52


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return GpuReducer(device=0)


def _es(dt):
    return torch.empty((), dtype=dt).element_size()


def _offsets(k, es):
    """Byte offsets past a 16-byte boundary of the wide and the 2-byte operand
    whose vectors first co-align after k elements."""
    return (16 - es * (k % (16 // es))) % 16, (16 - 2 * k) % 16


def _exact(n, wire, seed):
    """n wire values, small integers times powers of two: every square and
    every partial sum of squares is exact in f64, also after a divide by 8."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    m = torch.randint(-8, 9, (n,), generator=g, device="cuda").float()
    e = torch.randint(-2, 4, (n,), generator=g, device="cuda").float()
    return (m * torch.exp2(e)).to(wire)


def _random(n, wire, seed, lo=-12, hi=12):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, generator=g, device="cuda")
    x *= torch.exp2(torch.randint(lo, hi, (n,), generator=g, device="cuda").float())
    return x.to(wire)


def _put(x, where):
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

    def written(self, buf=None):
        """The segment's bytes of ``buf`` (default: W) on the host, as the wide dtype."""
        b = (self.W if buf is None else buf)[self.woff:self.woff + self.n * self.es].clone()
        return b.view(self.wide).cpu()

    def outside(self, buf=None):
        """The sentinel bytes in front of and behind the segment."""
        b = self.W if buf is None else buf
        return torch.cat([b[:self.woff], b[self.woff + self.n * self.es:]])


def _plan(red, segs, wire, kind):
    wide = segs[0].wide
    if kind == "ef":
        desc = [(s.wptr, s.hptr, s.n, s.rptr) for s in segs]
    elif kind == "sr":
        desc = [(s.wptr, s.hptr, s.n, SrKey(17 + i)) for i, s in enumerate(segs)]
    else:
        desc = [(s.wptr, s.hptr, s.n) for s in segs]
    return red.cast_plan(desc, from_torch(wide), from_torch(wire))


def _scaled_definition(plain, m):
    """torch CPU arithmetic on the plain decompress's output: ``* m`` in f32
    then the cast to the wide dtype, or the f64 product."""
    m32 = torch.tensor(m, dtype=F32)
    if plain.dtype == F64:
        return plain * m32.to(F64)
    if plain.dtype == F32:
        return plain * m32
    return (plain.to(F32) * m32).to(plain.dtype)


def _same_but_nan(got, want):
    """Bit for bit, NaN positions as NaN-ness only."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    if got.dtype != want.dtype or not torch.equal(gn, wn):
        return False
    as_int = {8: torch.int64, 4: torch.int32, 2: torch.int16}[got.element_size()]
    return torch.equal(got.contiguous().view(as_int)[~wn], want.contiguous().view(as_int)[~wn])


def _segments(wire, wide, kind="plain", maker=_exact, seed=0):
    """The smallest shapes that reach each path: one full tile, a partial tile,
    an element record from co-misaligned operands, a 0-element segment in the
    middle, and one segment of a head, two tiles and 5; +-inf and NaN on the
    wire at the edges, and (fp16) sums that overflowed to inf beside values
    that stay finite without a divide."""
    es = _es(wide)
    k = 3
    n2 = k + 2 * TILE + 5
    specs = [
        (_put(maker(TILE, wire, seed + 1), {0: INF, 7: NAN, TILE - 1: -INF}), 0, 0),
        (_put(maker(TILE - 3, wire, seed + 2), {0: NAN, -1: INF, 255 * 8: 60000.0}), 0, 0),
        (_put(maker(300, wire, seed + 3), {0: -INF, 299: NAN, 5: -60000.0}), 0, 2),
        (maker(0, wire, seed + 4), 0, 0),
        (_put(maker(n2, wire, seed + 5), {0: INF, k - 1: NAN, k: -INF, n2 - 1: INF,
                                           k + TILE: NAN, k + 2 * TILE: -INF}),
         *_offsets(k, es)),
    ]
    return [_Seg(v, wide, w, h, resid=(kind == "ef")) for v, w, h in specs]


MULTS = (1.0, 0.31415927410125732, 2.0 ** -7 * 0.7)


def _contract(red, segs, wire, divisor, kind="plain", mults=MULTS, report=""):
    """Measure and the scaled decompress of one plan against its own plain
    and statistics decompress; returns the rows."""
    cur = torch.cuda.current_stream()             # raw pointers name no device
    plan = _plan(red, segs, wire, kind)
    for s in segs:
        s.W.fill_(SENTINEL)
    want_rows = torch.full((2 * len(segs),), NAN, dtype=F64, device="cuda")
    plan.decompress(divisor, stream=cur, stats=want_rows)
    plain = [s.W.clone() for s in segs]
    halves = [s.H.clone() for s in segs]
    resid = [s.R.clone() for s in segs] if kind == "ef" else []
    # ---- measure
    rows = []
    for s in segs:
        s.W.fill_(SENTINEL)
    for launch in range(2):                       # a relaunch needs no reset
        st = torch.full((2 * len(segs),), NAN, dtype=F64, device="cuda")
        plan.measure(divisor, stream=cur, stats=st)
        rows.append(st.cpu())
    for s, h in zip(segs, halves):
        assert bool((s.W == SENTINEL).all()), "measure writes no byte of a wide buffer"
        assert torch.equal(s.H, h)
    assert not bool(torch.isnan(rows[0]).any()), "every row is overwritten"
    assert torch.equal(rows[0].view(torch.int64), rows[1].view(torch.int64)), "same bits twice"
    assert torch.equal(rows[0].view(torch.int64), want_rows.cpu().view(torch.int64)), \
        "the rows of decompress(stats=), bit for bit"
    # ---- scaled decompress
    for m in mults:
        mult = torch.tensor([m], dtype=F32, device="cuda")
        for s in segs:
            s.W.fill_(SENTINEL)
        plan.decompress(divisor, stream=cur, scale=mult)
        m_back = float(mult.cpu()[0])
        for i, (s, p) in enumerate(zip(segs, plain)):
            got, base = s.written(), s.written(p)
            want = _scaled_definition(base, m_back)
            assert _same_but_nan(got, want), (report, i, s.n, m)
            assert bool((s.outside() == SENTINEL).all()), "the sentinel bytes are intact"
            assert torch.equal(s.H, halves[i])
            if m == 1.0:
                assert _same_but_nan(got, base), "mult 1: the plain decompress's bytes"
                fin = ~torch.isnan(base)
                assert torch.equal(torch.isinf(got) & fin, torch.isinf(base) & fin)
    for s, r in zip(segs, resid):
        assert torch.equal(s.R, r)                # the residuals are not touched
    plan.close()
    return rows[0].view(-1, 2)


# ------------------------------------------------- measure + scaled decompress --
@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("wire,wide", PAIRS, ids=PAIR_IDS)
def test_measure_and_scaled_plain_plans(red, wire, wide, divisor):
    got = _contract(red, _segments(wire, wide), wire, divisor)
    assert got[3].tolist() == [0.0, 0.0]                      # nelem == 0, in the middle
    assert got[:, 1].tolist() == [3.0, 2.0, 2.0, 0.0, 6.0]    # +-inf and NaN, each once
    assert all(np.isfinite(got[:, 0].numpy()))
    _contract(red, _segments(wire, wide, maker=_random, seed=40), wire, divisor)


@pytest.mark.parametrize("kind", ["ef", "sr"])
@pytest.mark.parametrize("wire", [F16, BF16], ids=["fp16", "bf16"])
def test_measure_and_scaled_ef_and_sr_plans(red, wire, kind):
    for divisor in (1, 8):
        got = _contract(red, _segments(wire, F32, kind, maker=_random, seed=60), wire, divisor,
                        kind=kind)
        assert got[:, 1].tolist() == [3.0, 2.0, 2.0, 0.0, 6.0]


def test_overflow_on_the_wire_is_counted_not_added(red):
    """fp16 wire, no divide: a sum that overflowed is inf on the wire and is
    counted; 60000 and 65504 stay finite and enter the sum."""
    v = torch.tensor([60000.0, INF, 2.0, 65504.0, -INF], dtype=F16, device="cuda")
    got = _contract(red, [_Seg(v, F32)], F16, 1)
    assert got[0].tolist() == [60000.0 ** 2 + 4.0 + 65504.0 ** 2, 2.0]
    # bf16 wire into fp16: 99840 overflows the WIDE type unless divided first
    v = torch.tensor([99840.0, 2.0, -99840.0], dtype=BF16, device="cuda")
    assert _contract(red, [_Seg(v.clone(), F16)], BF16, 1)[0].tolist() == [4.0, 2.0]
    assert _contract(red, [_Seg(v.clone(), F16)], BF16, 8)[0].tolist() == \
        [2 * 12480.0 ** 2 + 0.0625, 0.0]


def test_scaled_products_that_become_subnormal(red):
    """f32 products below 2^-126 (bf16 wire into f32), and products that round
    to fp16 / bf16 subnormals in the 2-byte wide types."""
    n = TILE + 2 * 8 + 5
    cases = [
        # bf16 values around 2^-120 times 1.3 * 2^-10: f32 subnormals
        (BF16, F32, _random(n, BF16, 1, -124, -116), 1.3 * 2.0 ** -10),
        # bf16 values around 2^-10 times 1.3 * 2^-10: fp16 subnormals (below 2^-14)
        (BF16, F16, _random(n, BF16, 2, -12, -8), 1.3 * 2.0 ** -10),
        # fp16 values around 2^-10 times 1.3 * 2^-120: bf16 subnormals (below 2^-126)
        (F16, BF16, _random(n, F16, 3, -12, -8), 1.3 * 2.0 ** -120),
    ]
    for wire, wide, v, m in cases:
        seg = _Seg(v, wide, *_offsets(3, _es(wide)))
        _contract(red, [seg], wire, 1, mults=(m,))
        out = seg.written().to(F64)
        tiny = {F32: 2.0 ** -126, F16: 2.0 ** -14, BF16: 2.0 ** -126}[wide]
        sub = (out.abs() < tiny) & (out != 0)
        assert int(sub.sum()) > n // 4, "the case reaches subnormal products"


# ------------------------------------------------------------------- record --
def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _check_record(red, rows, max_norm, eps, inv, exact, out=None):
    """One clip record against the definition on the same rows."""
    inv_t = None if inv is None else torch.tensor([inv], dtype=F32, device="cuda")
    rec = red.clip_record(rows, max_norm, eps, inv_t, out=out)
    raw = rec.tensor.cpu()
    sumsq, nonfinite, norm = raw.view(F64)[:3].tolist()
    coef, mult = raw.view(F32)[6:8].tolist()
    assert [float(rec.sumsq), float(rec.nonfinite), float(rec.norm), float(rec.coef),
            float(rec.mult)] == [sumsq, nonfinite, norm, coef, mult], "the views name the fields"
    want = compression.clip_record(rows.cpu(), max_norm, eps, inv)
    nrows = rows.numel() // 2
    print(f"record nrows={nrows} sumsq {sumsq!r} ref {float(want.sumsq)!r} norm {norm!r} "
          f"coef {coef!r} ref {float(want.coef)!r} mult {mult!r} ref {float(want.mult)!r}")
    assert nonfinite == float(want.nonfinite)
    if exact:
        assert sumsq == float(want.sumsq)
    else:
        assert abs(sumsq - float(want.sumsq)) <= nrows * EPS52 * float(want.sumsq)
    inv64 = 1.0 if inv is None else float(np.float32(inv))
    norm_def = float(np.sqrt(np.float64(sumsq)) * np.float64(inv64))
    assert abs(norm - norm_def) <= 4 * EPS52 * norm_def
    assert abs(coef - float(want.coef)) <= _ulp32(float(want.coef))
    assert abs(mult - float(want.mult)) <= _ulp32(float(want.mult))
    return rec, (sumsq, nonfinite, norm, coef, mult)


@pytest.mark.parametrize("inv", [None, 2.0 ** -16], ids=["noscale", "inv2^-16"])
def test_record_of_a_plans_rows(red, inv):
    cur = torch.cuda.current_stream()
    for maker, exact in ((_exact, True), (_random, False)):
        segs = _segments(F16, F32, maker=maker, seed=80)
        plan = _plan(red, segs, F16, "plain")
        rows = torch.full((2 * len(segs),), NAN, dtype=F64, device="cuda")
        plan.measure(8, stream=cur, stats=rows)
        total = float(rows.cpu().view(-1, 2)[:, 0].sum().sqrt()) * (inv or 1.0)
        # norm above max_norm: the clip bites; non-finite values are present
        _, (_, nf, norm, coef, mult) = _check_record(red, rows, total / 3, 1e-6, inv, exact)
        assert nf == 13.0 and np.isfinite(norm) and 0.33 < coef < 0.3334
        # norm below max_norm: coef is 1 exactly and mult is inv_scale, bit for bit
        _, (_, _, _, coef, mult) = _check_record(red, rows, total * 3, 1e-6, inv, exact)
        assert coef == 1.0 and mult == (1.0 if inv is None else inv)
        plan.close()


def test_record_edge_rows(red):
    dev = dict(dtype=F64, device="cuda")
    # no rows: sumsq 0, coef 1
    rec, got = _check_record(red, torch.empty(0, **dev), 1.0, 1e-6, None, True)
    assert got == (0.0, 0.0, 0.0, 1.0, 1.0)
    _, got = _check_record(red, torch.empty((0, 2), **dev), 2.5, 0.0, 0.25, True, out=rec)
    assert got == (0.0, 0.0, 0.0, 1.0, 0.25)
    # all-zero gradients, eps 0 included: max_norm / 0 is +inf, coef 1
    for eps in (1e-6, 0.0):
        _, got = _check_record(red, torch.zeros((5, 2), **dev), 1.0, eps, 2.0 ** -16, True)
        assert got == (0.0, 0.0, 0.0, 1.0, 2.0 ** -16)
    # more rows than the workgroup has lanes, counts that need more than 32 bits
    g = torch.Generator(device="cuda").manual_seed(5)
    rows = torch.rand((3000, 2), generator=g, **dev)
    rows[:, 1] = torch.randint(0, 2 ** 40, (3000,), generator=g, device="cuda").to(F64)
    _check_record(red, rows, 7.0, 1e-6, None, False)
    _check_record(red, rows, 7.0, 1e-6, 2.0 ** -16, False)
    # exact sums over many rows
    rows = torch.randint(0, 2 ** 20, (2500, 2), generator=g, device="cuda").to(F64)
    _check_record(red, rows, 3.0, 1e-6, 0.5, True)


# ------------------------------------------------------------------- errors --
def test_bad_arguments_raise_before_any_launch(red):
    cur = torch.cuda.current_stream()
    lib, stream = red.lib, int(cur.cuda_stream)
    segs = [_Seg(_exact(TILE + 9, F16, 31), F64), _Seg(_exact(100, F16, 32), F64)]
    plan = _plan(red, segs, F16, "plain")
    before = [s.W.clone() for s in segs]
    ok = torch.zeros(4, dtype=F64, device="cuda")
    one = torch.ones(4, dtype=F32, device="cuda")
    s0 = segs[0]

    def eargs(call, *a, **kw):
        with pytest.raises(reducer.ReduceError) as e:
            call(*a, **kw)
        assert e.value.code == reducer.EARGS

    # measure: _decompress_stats's rules
    eargs(plan.measure, 1, cur, s0.W[s0.woff:s0.woff + 32].view(F64))   # inside a wide range
    eargs(plan.measure, 1, cur, s0.wptr - 24)                # reaches 8 bytes into it
    eargs(plan.measure, 1, cur, segs[1].hptr)                # a 2-byte side
    eargs(plan.measure, 1, cur, ok.data_ptr() + 4)           # not 8-byte aligned
    eargs(plan.measure, 1, cur, 0)                           # null
    eargs(plan.measure, 0, cur, ok)                          # divisor < 1
    assert lib.byteps_reduce_cast_plan_measure(None, 1, ok.data_ptr(), stream) == reducer.EARGS
    with pytest.raises(ValueError):
        plan.measure(1, cur, None)
    with pytest.raises(ValueError):
        plan.measure(1, cur, torch.zeros(4, device="cuda"))                 # dtype
    with pytest.raises(ValueError):
        plan.measure(1, cur, torch.zeros(6, dtype=F64, device="cuda"))      # size
    # scaled decompress
    eargs(plan.decompress, 1, cur, scale=0)                  # null mult
    eargs(plan.decompress, 1, cur, scale=one.data_ptr() + 2)  # not 4-byte aligned
    eargs(plan.decompress, 0, cur, scale=one[:1])            # divisor < 1
    eargs(plan.decompress, 1, cur, scale=s0.wptr)            # first bytes of a wide range
    eargs(plan.decompress, 1, cur, scale=s0.wptr + s0.n * 8 - 4)            # its last 4 bytes
    eargs(plan.decompress, 1, cur, scale=segs[1].hptr + 4)   # inside a 2-byte side
    assert lib.byteps_reduce_cast_plan_decompress_scaled(None, 1, one.data_ptr(), stream) == \
        reducer.EARGS
    with pytest.raises(ValueError):
        plan.decompress(1, cur, stats=ok, scale=one[:1])     # stats together with scale
    with pytest.raises(ValueError):
        plan.decompress(1, cur, scale=one)                   # four elements
    with pytest.raises(ValueError):
        plan.decompress(1, cur, scale=ok[:1])                # float64
    with pytest.raises(ValueError):
        plan.decompress(1, cur, scale=torch.ones(1))         # on the host
    # clip record
    rec = torch.full((48,), SENTINEL, dtype=torch.uint8, device="cuda")
    rp, op = ok.data_ptr(), rec.data_ptr()
    f = lib.byteps_reduce_clip_record
    assert f(None, 2, 1.0, 1e-6, None, op, stream) == reducer.EARGS        # null rows, nrows > 0
    assert f(rp, -1, 1.0, 1e-6, None, op, stream) == reducer.EARGS         # nrows < 0
    assert f(rp, 2, 1.0, 1e-6, None, None, stream) == reducer.EARGS        # null out
    assert f(rp, 2, 1.0, 1e-6, None, op + 4, stream) == reducer.EARGS      # misaligned out
    for bad in (0.0, -1.0, INF, NAN):
        assert f(rp, 2, bad, 1e-6, None, op, stream) == reducer.EARGS      # max_norm
    assert f(rp, 2, 1.0, -1e-9, None, op, stream) == reducer.EARGS         # eps < 0
    assert f(rp, 2, 1.0, NAN, None, op, stream) == reducer.EARGS
    with pytest.raises(ValueError):
        red.clip_record(torch.zeros(4, device="cuda"), 1.0)                # dtype
    with pytest.raises(ValueError):
        red.clip_record(torch.zeros(3, dtype=F64, device="cuda"), 1.0)     # odd
    with pytest.raises(ValueError):
        red.clip_record(ok, 1.0, inv_scale=torch.ones(1))                  # inv_scale on the host
    torch.cuda.synchronize()
    for s, b in zip(segs, before):
        assert torch.equal(s.W, b)                           # nothing ran
    assert ok.tolist() == [0.0] * 4 and one.tolist() == [1.0] * 4
    assert bool((rec == SENTINEL).all())
    # touching ranges are fine: a multiplier right in front of a wide range
    front = s0.W[s0.woff - 4:s0.woff].view(F32)
    front.fill_(0.5)
    plan.decompress(1, stream=cur, scale=front)
    torch.cuda.synchronize()
    assert float(front[0]) == 0.5
    plan.close()
    # plans without records: nothing to launch, measure still writes its rows
    empty = red.cast_plan([], from_torch(F32))
    empty.measure(1, stream=cur, stats=torch.empty(0, dtype=F64, device="cuda"))
    empty.decompress(1, stream=cur, scale=one[:1])
    empty.close()
    st = torch.full((4,), NAN, dtype=F64, device="cuda")
    hollow = red.cast_plan([(0, 0, 0), (0, 0, 0)], from_torch(F32))
    hollow.measure(3, stream=cur, stats=st)
    hollow.decompress(3, stream=cur, scale=one[:1])
    torch.cuda.synchronize()
    assert st.tolist() == [0.0] * 4
    hollow.close()


# -------------------------------------------------------------- compressors --
@pytest.mark.parametrize("name", ["fp16", "bf16_ef", "fp16_sr"])
def test_compressors_clip_on_the_device(name):
    """decompress_many_into(clip_norm=): measure, record and scaled decompress
    over cached plans; ``stats`` receives the rows before the clip."""
    from prophet_amd.compression import CastPlanCache, Compression
    comp = getattr(Compression, name)
    wire = comp.wire_torch_dtype()
    dts = [F32, F32, F32, F32] if name != "fp16" else [F32, F64, F32, BF16]
    sizes = [300, TILE + 9, 0, 2 * TILE]
    outs = [torch.empty(n, dtype=dt, device="cuda") for n, dt in zip(sizes, dts)]
    ws = [_put(_random(n, wire, 40 + i, -3, 3), {1: INF}) for i, n in enumerate(sizes)]
    extra = {}
    if name.endswith("_ef"):
        extra["residuals"] = [comp.residual_like(o) for o in outs]
    if name.endswith("_sr"):
        extra["keys"] = [7, 8, 9, 10]
    cache = CastPlanCache(4)
    plain = [torch.empty_like(o) for o in outs]
    want_rows = torch.empty((4, 2), dtype=F64, device="cuda")
    comp.decompress_many_into(plain, ws, 8, plans=cache, stats=want_rows, **extra)
    built = None
    for unscale in (2.0 ** -7, torch.tensor([2.0 ** -7], dtype=F32, device="cuda")):
        for o in outs:
            o.fill_(-77.0)
        st = torch.full((4, 2), NAN, dtype=F64, device="cuda")
        total = float(want_rows[:, 0].sum().sqrt()) * 2.0 ** -7
        rec = comp.decompress_many_into(outs, ws, 8, plans=cache, stats=st, clip_norm=total / 2,
                                        unscale=unscale, **extra)
        assert isinstance(rec, reducer.ClipRecord)
        assert torch.equal(st.view(torch.int64), want_rows.view(torch.int64)), "pre-clip rows"
        want = compression.clip_record(st.cpu(), total / 2, 1e-6, 2.0 ** -7)
        m = float(rec.mult)
        assert abs(m - float(want.mult)) <= _ulp32(float(want.mult)) and m < 2.0 ** -7
        assert float(rec.nonfinite) == 3.0
        for o, p in zip(outs, plain):
            assert _same_but_nan(o.cpu(), _scaled_definition(p.cpu(), m))
        # a second round reuses the plans of the first
        built = built or cache.built
        assert cache.built == built
    # measure_many_with writes nothing to the outputs
    for o in outs:
        o.fill_(-77.0)
    st = torch.full((4, 2), NAN, dtype=F64, device="cuda")
    comp.measure_many_with(outs, ws, None, 8, cache, st)
    assert torch.equal(st.view(torch.int64), want_rows.view(torch.int64))
    assert all(bool((o == -77.0).all()) for o in outs)
    # without a cache the plans are built and destroyed inside the call
    rec = comp.decompress_many_into(outs[:1], ws[:1], 1, clip_norm=1e9)
    assert float(rec.coef) == 1.0 and float(rec.mult) == 1.0
    comp.decompress_into(plain[0], ws[0], 1)
    assert _same_but_nan(outs[0].cpu(), plain[0].cpu())
    with pytest.raises(ValueError):
        comp.decompress_many_into(outs, ws, 8, unscale=0.5)                 # no clip_norm
    with pytest.raises(ValueError):
        comp.decompress_many_into(outs, ws, 8, clip_norm=0.0)
    with pytest.raises(ValueError):
        comp.decompress_many_into([outs[0], torch.empty(9)], [ws[0], torch.empty(9, dtype=wire)],
                                  8, clip_norm=1.0)                          # two places
    cache.close()


# -------------------------------------------------------- larger tile sizes --
def _tile_case(red, u, wire, wide):
    """One plan just over the size where the tile-size rule picks u units a
    lane (kMinTiles tiles of kBlock * u units, with the library's copy tile at
    u), a head, a partial tile and a tail behind it, a small segment beside
    it."""
    k = 3
    n = k + (K_MIN_TILES + 1) * u * TILE + 3 * 8 + 5
    where = {0: INF, k: NAN, k + u * TILE - 1: -INF, n - 1: NAN,
             k + K_MIN_TILES * u * TILE: INF, k + (K_MIN_TILES + 1) * u * TILE + 9: -INF}
    wo, ho = _offsets(k, _es(wide))
    segs = [_Seg(_put(_random(n, wire, 60 + u, -3, 3), where), wide, wo, ho),
            _Seg(_random(1000, wire, 61), wide)]
    got = _contract(red, segs, wire, 8, mults=(0.31415927410125732,), report=f"u={u}")
    assert got[:, 1].tolist() == [float(len(where)), 0.0]


@pytest.mark.parametrize("u", [2, 4])
def test_larger_tiles_in_a_child_process(u):
    env = dict(os.environ, BPSR_COPY_VPT=str(u))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(u)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{u}-unit cases passed" in r.stdout


if __name__ == "__main__":
    _u = int(sys.argv[1])
    _red = GpuReducer(device=0)
    for _wire, _wide in PAIRS:
        _tile_case(_red, _u, _wire, _wide)
    print(f"{_u}-unit cases passed")
