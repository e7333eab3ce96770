"""Cast plans (byteps_reduce_cast_plan_*, prophet_amd/csrc/bpsr_k_cast_plan.hip)
on the GPU: one launch over many segments against the one-tensor calls (bit
for bit, sentinel bytes between the segments intact) and against the host
(CPU torch casts and ``div_`` on the fp16 tensor; where the host has a NaN
only a NaN is required), the launch shapes with 2 and 4 units per lane and
non-temporal stores, the bounds check, empty plans, and
``push_pull_iteration(average=True)`` over the real server with exactly one
plan launch each way per worker and iteration.

The tile size comes from the library's tuning, which a process reads once
(copy tile of 2 units unless BPSR_COPY_VPT says otherwise), so the 4-unit
shape runs in a child process started with BPSR_COPY_VPT=4: this file, run as
a script."""
import os
import subprocess
import sys
import threading
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from prophet_amd import reducer  # noqa: E402
from prophet_amd.dtypes import DType, from_torch  # noqa: E402
from prophet_amd.reducer import GpuReducer  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

WIDE = [torch.float32, torch.float64, torch.bfloat16]
IDS = ["f32", "f64", "bf16"]
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
    """Elements of ``got`` that differ from the host's ``want``: other bits
    where want is a number, not a NaN where want is one."""
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
    """f64 values whose first 64 hold what the casts must get right: fp16
    overflow, subnormal results, ties (midpoints of two fp16 values, exact in
    f32 but not bf16), signed zeros and one NaN."""
    rng = np.random.default_rng(31)
    x = rng.standard_normal(n) * np.exp2(rng.integers(-27, 17, n))
    special = [65504.0, 65519.996, 65520.0, -7e4, 1e38, 1e-7, -3e-8, 2.0 ** -25, 2.0 ** -24 * 1.5,
               0.0, -0.0, 1 + 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 3 * 2.0 ** -11, 6.1e-5, -6.0e-5,
               float("nan"), 2049.0, 2051.0, -4098.0, 3.0, 1 / 3]
    x[:len(special)] = special
    x[len(special):64:3] = 65519.0                     # rounds down to 65504; / 3 is inexact
    return x


# (elements, wide offset, fp16 offset) with the offsets in BYTES past a
# 256-byte boundary.  Every size of the table test at three pairs of element
# offsets each — pairs that co-align after a head and pairs that never do —
# then element-misaligned operands and a never-co-aligning segment of three
# element parts.
def _layout(es):
    sizes = (0, 1, 7, 8, 9, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
    offs = (0, 1, 3)
    segs = []
    for k in range(3):
        for j, n in enumerate(sizes):
            segs.append((n, offs[k] * es, offs[(j + k) % 3] * 2))
    segs += [(TILE + 1, 1, 0), (9, 0, 1), (TILE + 1, es, 3), (10000, 0, 2)]
    return segs


class _Arenas:
    """The segments of `_layout` in one arena per side."""

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
        """The bytes of an arena of `nbytes` that belong to a segment."""
        m = torch.zeros(nbytes, dtype=torch.bool)
        for (n, _, _), o in zip(self.layout, offs):
            m[o:o + n * width] = True
        return m


@pytest.mark.parametrize("dt", WIDE, ids=IDS)
def test_segments_offsets_tails_and_sentinels(red, dt):
    lay = _Arenas(dt, _layout(torch.empty((), dtype=dt).element_size()))
    es, dtype = lay.es, from_torch(dt)
    nmax = max(n for n, _, _ in lay.layout)
    base = torch.from_numpy(_values(nmax + 64)).to(dt)
    base_bytes = base.view(torch.uint8).cuda()
    starts = [(5 * i) % 64 for i in range(len(lay.layout))]
    W, H = _arena(lay.wbytes), _arena(lay.hbytes)
    for (n, _, _), o, s in zip(lay.layout, lay.woff, starts):
        W[o:o + n * es] = base_bytes[s * es:(s + n) * es]
    W_in = W.clone()
    segs = [(W.data_ptr() + wo, H.data_ptr() + ho, n)
            for (n, _, _), wo, ho in zip(lay.layout, lay.woff, lay.hoff)]
    segs.insert(3, (0, 0, 0))                              # no pointers, no elements
    plan = red.cast_plan(segs, dtype)
    cur = torch.cuda.current_stream()                      # raw pointers name no device
    # compress: against one call per segment into an arena laid out the same
    plan.compress(stream=cur)
    H_one = _arena(lay.hbytes)
    for (n, _, _), wo, ho in zip(lay.layout, lay.woff, lay.hoff):
        red.compress_fp16(H_one.data_ptr() + ho, W.data_ptr() + wo, n, dtype,
                          stream=cur)
    assert torch.equal(H, H_one)
    assert torch.equal(W, W_in)
    Hc = H.cpu()
    assert bool((Hc[~lay.mask(lay.hbytes, lay.hoff, 2)] == SENTINEL).all())
    halves = []
    nans = 0
    for (n, _, _), ho, s in zip(lay.layout, lay.hoff, starts):
        want = base[s:s + n].to(torch.float16)
        got = Hc[ho:ho + 2 * n].clone().view(torch.float16)
        assert _mismatches(got, want) == 0, (n, ho)
        halves.append(want)
        nans += int(torch.isnan(want).sum())
    assert nans >= 3                                       # the NaN is in several segments
    allh = torch.cat(halves)
    assert int(torch.isinf(allh).sum()) > 50 and int(((_bits(allh) & 0x7c00) == 0).sum()) > 50
    # decompress: the plan writes the wide arena it was built over
    for divisor in (1, 3):
        W.fill_(SENTINEL)
        plan.decompress(divisor, stream=cur)
        W_one = _arena(lay.wbytes)
        for (n, _, _), wo, ho in zip(lay.layout, lay.woff, lay.hoff):
            red.decompress_fp16(W_one.data_ptr() + wo, H.data_ptr() + ho, n, dtype, divisor,
                                stream=cur)
        assert torch.equal(W, W_one), divisor
        assert torch.equal(H, H_one)
        Wc = W.cpu()
        assert bool((Wc[~lay.mask(lay.wbytes, lay.woff, es)] == SENTINEL).all())
        for (n, _, _), wo, ho in zip(lay.layout, lay.woff, lay.hoff):
            # the host's input is what the device wrote (NaN payloads included)
            h = Hc[ho:ho + 2 * n].clone().view(torch.float16)
            want = (h.clone().div_(divisor) if divisor > 1 else h).to(dt)
            got = Wc[wo:wo + n * es].clone().view(dt)
            assert _mismatches(got, want) == 0, (divisor, n, wo)
    plan.close()
    plan.close()                                           # idempotent


def _big_case(red, total, report=None):
    """One f32 plan of `total` elements and more: a few large segments at odd
    offsets plus small odd ones.  Everything is compared on the device: with
    the one-tensor kernels (which tests/test_compress_gpu.py pins to the
    host) and with torch's device arithmetic, IEEE like the host's; a slice
    of each large segment also goes to the host."""
    g = torch.Generator(device="cuda").manual_seed(41)
    big = [total // 2 + 13, total // 4 + 4096 + 11, total // 4]
    small = [7, 4097, 1, 3 * TILE + 5]
    xs, hs = [], []
    for i, n in enumerate(big + small):
        k = i % 4               # both sides k elements in: they co-align after 0, 7, 6, 5
        x = torch.randn(n + 8, generator=g, device="cuda")
        x *= torch.exp2(torch.randint(-20, 17, (n + 8,), generator=g, device="cuda").float())
        xs.append(x[k:k + n])
        hs.append(torch.empty(n + 8, dtype=torch.float16, device="cuda")[k:k + n])
    assert sum(big + small) >= total
    plan = red.cast_plan([(x, h, x.numel()) for x, h in zip(xs, hs)], DType.FLOAT32)
    plan.compress()
    three = torch.full((), 3.0, device="cuda")             # a device divisor: a true divide
    for x, h in zip(xs, hs):
        one = torch.empty_like(h)
        red.compress_fp16(one, x, x.numel(), DType.FLOAT32)
        assert torch.equal(_bits(h), _bits(one))
        assert torch.equal(_bits(h), _bits(x.to(torch.float16)))
    xin = [x.clone() for x in xs]
    for x in xs:
        x.fill_(-1.0)
    plan.decompress(3)
    for x, h, x0 in zip(xs, hs, xin):
        one = torch.empty_like(x)
        red.decompress_fp16(one, h, x.numel(), DType.FLOAT32, 3)
        assert torch.equal(_bits(x), _bits(one))
        assert torch.equal(_bits(x), _bits((h.float() / three).to(torch.float16).float()))
        m = min(x.numel(), 100_000)
        hw = x0[-m:].cpu().to(torch.float16)
        assert torch.equal(_bits(h[-m:].cpu()), _bits(hw))
        assert torch.equal(_bits(x[-m:].cpu()), _bits(hw.div_(3).float()))
    plan.close()
    if report:
        print(report)


# 2 units per lane from 2048 such tiles on: 2048 * 2 * TILE = 8 Mi elements
# (write-through stores: 32 MiB of f32).  From 96 MiB of output on the stores
# are non-temporal: 32 Mi elements decompress into 128 MiB of f32.
@pytest.mark.parametrize("total", [8 << 20, 32 << 20], ids=["2units_wt", "2units_nt"])
def test_tile_sizes_and_store_policy(red, total):
    _big_case(red, total)


def test_four_unit_tiles_in_a_child_process():
    """BPSR_COPY_VPT=4 and 32 Mi elements (4096 tiles of 4 units): the plan is
    cut for 4 units per lane, with non-temporal stores one way."""
    env = dict(os.environ, BPSR_COPY_VPT="4")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "four-unit case passed" in r.stdout


def test_short_operand_raises_before_any_launch(red):
    wide = torch.zeros(1000, device="cuda")
    half = torch.zeros(1000, dtype=torch.float16, device="cuda")
    ok = (torch.ones(64, device="cuda"), torch.zeros(64, dtype=torch.float16, device="cuda"), 64)
    for seg in [(wide, half[:999], 1000), (wide[:999], half, 1000)]:
        with pytest.raises(ValueError):
            red.cast_plan([ok, seg], DType.FLOAT32)
    with pytest.raises(ValueError):
        red.cast_plan([ok, (wide, half, 1000)], DType.FLOAT64)     # 4000 bytes: 500 doubles
    torch.cuda.synchronize()
    assert float(half.abs().sum()) == 0.0 and float(ok[1].abs().sum()) == 0.0


def test_empty_plans_launch_nothing(red):
    e = torch.empty(0, device="cuda")
    eh = torch.empty(0, dtype=torch.float16, device="cuda")
    for segs in ([], [(0, 0, 0)], [(e, eh, 0), (0, 0, 0), (e, eh, 0)]):
        for dt in (DType.FLOAT32, DType.FLOAT64, DType.BFLOAT16):
            plan = red.cast_plan(segs, dt)
            plan.compress()
            plan.decompress()
            plan.decompress(5)
            with pytest.raises(reducer.ReduceError):
                plan.decompress(0)
            plan.close()
    torch.cuda.synchronize()


# ------------------------------------------------------------- end to end --
N, ITERS = 3, 2
NELEMS = [1, 7, 4097, 32768 + 3, 2 * 32768 + 4097]
NAMES = [f"g{i}" for i in range(len(NELEMS))]


def _grad(rank, it, i):
    n = NELEMS[i]
    rng = np.random.default_rng(1000 * it + 10 * rank + i)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-4, 12, n))).astype(np.float32)
    if n > 100:
        # past fp16's range (one sign per index on every worker: no inf - inf,
        # so no NaN), and inside its subnormal range
        x[0:16] = 7e4 + rank
        x[16:32] = -(65520.0 + 100 * rank)
        x[32:48] = 65519.0 - rank
        x[48:64] = (np.arange(16) + 1 + rank) * np.float32(2.0 ** -25)
        x[64:80] = -(np.arange(16) + 3 * rank) * np.float32(3e-8)
        x[80:84] = [0.0, -0.0, 6.1e-5, -6.0e-5]
    return x


@pytest.mark.parametrize("prophet", [False, True], ids=["fifo", "prophet"])
def test_iteration_casts_once_each_way(monkeypatch, prophet):
    from oracle.oracle import PortReducer
    from prophet_amd.compression import Compression
    from prophet_amd.prophet import ProphetPushQueue
    from prophet_amd.pushpull import ServerFrontend, Worker
    from prophet_amd.server import PSServer
    assert torch.cuda.is_available()
    ops = ("compress", "decompress", "compress_fp16", "decompress_fp16")
    # every key made here: the worker threads only add to existing entries
    calls = Counter({(f"w{r}", op): 0 for r in range(N) for op in ops})

    def counted(cls, name):
        orig = getattr(cls, name)

        def wrapper(self, *a, **kw):
            calls[(threading.current_thread().name, name)] += 1
            return orig(self, *a, **kw)
        monkeypatch.setattr(cls, name, wrapper)
    counted(reducer.CastPlan, "compress")
    counted(reducer.CastPlan, "decompress")
    counted(reducer.GpuReducer, "compress_fp16")
    counted(reducer.GpuReducer, "decompress_fp16")

    srv = PSServer(N)
    fe = ServerFrontend(srv)
    workers = [Worker(r, fe, partition_bytes=64 << 10) for r in range(N)]
    data = {(r, it): [_grad(r, it, i) for i in range(len(NELEMS))]
            for r in range(N) for it in range(ITERS + 1)}
    held = {r: {nm: torch.from_numpy(data[(r, 1)][i]).cuda() for i, nm in enumerate(NAMES)}
            for r in range(N)}
    MOVED_RANK, MOVED = 1, "g2"
    bar = threading.Barrier(N + 1)
    errors, seen = [], {}

    def run(w):
        try:
            me = threading.current_thread().name
            for nm in NAMES:
                w.declare(nm)
            for i, nm in enumerate(NAMES):
                ctx = w.init_tensor(nm, torch.from_numpy(data[(w.rank, 0)][i]).cuda(),
                                    DType.FLOAT32, compression=Compression.fp16)
                assert ctx.dtype == DType.FLOAT16 and ctx.size == 2 * NELEMS[i]
            for it in range(1, ITERS + 1):
                if it > 1:
                    for i, nm in enumerate(NAMES):
                        fresh = torch.from_numpy(data[(w.rank, it)][i]).cuda()
                        if w.rank == MOVED_RANK and nm == MOVED:
                            assert fresh.data_ptr() != held[w.rank][nm].data_ptr()
                            held[w.rank][nm] = fresh      # the old one lives on in the cached plan
                        else:
                            held[w.rank][nm].copy_(fresh)
                before = Counter(calls)
                q = ProphetPushQueue(64, 1000, 1 << 18, checkpoints=(-1, 1, 4),
                                     backward_exec=(2, 5, 0)) if prophet else None
                w.push_pull_iteration(held[w.rank], scheduler=q, average=True)
                torch.cuda.current_stream().synchronize()
                seen[(w.rank, it)] = (
                    {k[1]: calls[k] - before[k] for k in calls if k[0] == me},
                    w._cast_plans.built)
                bar.wait(timeout=60)             # main thread reads arrival orders
                bar.wait(timeout=60)
        except Exception as e:  # surfaced below
            errors.append(repr(e))
            bar.abort()

    ts = [threading.Thread(target=run, args=(w,), name=f"w{w.rank}") for w in workers]
    for t in ts:
        t.start()
    port = PortReducer(nthreads=4)
    try:
        for it in range(1, ITERS + 1):
            bar.wait(timeout=120)
            ctxs = workers[0].contexts
            assert [ln for _, _, ln in ctxs["g4"].parts] == [65536, 65536, 2 * 4097]
            orders = {key: srv.key_info(key)[2] for nm in NAMES for key, _, _ in ctxs[nm].parts}
            got = {r: {nm: held[r][nm].cpu().numpy() for nm in NAMES} for r in range(N)}
            bar.wait(timeout=60)
            for i, nm in enumerate(NAMES):
                halves = {r: torch.from_numpy(data[(r, it)][i]).to(torch.float16).numpy()
                          .view(np.uint8) for r in range(N)}
                for key, off, ln in ctxs[nm].parts:
                    order = orders[key]
                    assert sorted(order) == list(range(N))
                    folded = np.zeros(ln, np.uint8)
                    assert port.sum_n(folded, [halves[r][off:off + ln].copy() for r in order],
                                      ln, DType.FLOAT16) == 0
                    q = torch.from_numpy(folded.view(np.float16).copy()).div_(N)
                    want = q.to(torch.float32).numpy()
                    assert not np.isnan(want).any()
                    if nm == "g4" and off == 0:
                        assert np.isinf(want[:32]).all() and (want[48:64] != 0).any()
                    for r in range(N):
                        g = got[r][nm][off // 2:(off + ln) // 2]
                        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), \
                            (it, nm, key, r)
    except threading.BrokenBarrierError:
        pass                                     # a worker failed: reported below
    except BaseException:
        bar.abort()                              # let the workers go, then fail
        raise
    for t in ts:
        t.join(timeout=60)
    assert not errors, errors
    for (r, it), (ops, built) in sorted(seen.items()):
        # one plan launch each way, and no one-tensor cast
        assert ops.get("compress", 0) == 1 and ops.get("decompress", 0) == 1, (r, it, ops)
        assert ops.get("compress_fp16", 0) == 0 and ops.get("decompress_fp16", 0) == 0, (r, it, ops)
        # one plan serves both ways and the next iteration; the worker whose
        # gradient moved builds exactly one more
        assert built == (2 if it == 2 and r == MOVED_RANK else 1), (r, it, built)
    for w in workers:
        w.close()
        assert len(w._cast_plans) == 0
    srv.close()


if __name__ == "__main__":
    _big_case(GpuReducer(device=0), 32 << 20, report="four-unit case passed")
