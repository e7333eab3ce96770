"""push_pull with ``Compression.bf16`` over the real GPU-resident server: 3
worker threads, f32 tensors travelling as bf16 (three partitions, the last
odd-sized), folded by the server's bf16 kernel, averaged on the bf16 value and
widened by one fused launch.  Every worker's every bit equals the host's
``widen(div_bf16(fold_bf16(compress(x_r))))`` in the server's recorded arrival
order: CPU torch casts and ``div_``, the oracle's bf16 fold.  Gradients past
fp16's range come back finite — through ``Compression.fp16`` the same inputs
are inf — and one ``push_pull_iteration`` mixes an uncompressed, an fp16 and a
bf16 context."""
import threading

import numpy as np
import pytest

from oracle.oracle import PortReducer
from prophet_amd.compression import Compression
from prophet_amd.dtypes import DType

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

N, ITERS = 3, 2
NELEM = 2 * 32768 + 4097
WIRE = {"none": (DType.FLOAT32, None), "fp16": (DType.FLOAT16, torch.float16),
        "bf16": (DType.BFLOAT16, torch.bfloat16)}


def _grad(rank, it):
    rng = np.random.default_rng(100 * it + rank)
    x = (rng.standard_normal(NELEM) * np.exp2(rng.integers(-4, 12, NELEM))).astype(np.float32)
    # past fp16's range (one sign per index on every worker), f32 subnormals
    # (kept by the bf16 cast, zero as fp16) and signed zeros
    x[0:16] = 7e4 + rank
    x[16:32] = -(65520.0 + 100 * rank)
    x[32:48] = 65519.0 - rank
    x[48:64] = ((np.arange(16) + 1 + rank) * 0x8001).astype(np.uint32).view(np.float32)
    x[64:80] = -((np.arange(16) + 3 * rank + 1) * 0x10000).astype(np.uint32).view(np.float32)
    x[80:84] = [0.0, -0.0, 6.1e-5, -6.0e-5]
    return x


def _expected(port, xs, order, off, ln, wire, average):
    """The host's result for one partition: bytes [off, off + ln) of the WIRE
    tensor, as f32.  ``xs``: every rank's f32 gradient."""
    dtype, tdt = WIRE[wire]
    if tdt is None:
        parts = [x.view(np.uint8)[off:off + ln].copy() for x in xs]
    else:
        parts = [torch.from_numpy(x).to(tdt).view(torch.int16).numpy().view(np.uint8)
                 [off:off + ln].copy() for x in xs]
    folded = np.zeros(ln, np.uint8)
    assert port.sum_n(folded, [parts[r] for r in order], ln, dtype) == 0
    if tdt is None:
        # an uncompressed context is averaged by torch on the device, which is
        # not this file's subject: the same call, not the host's divide
        q = torch.from_numpy(folded.view(np.float32).copy())
        return (q.cuda().div_(N).cpu() if average else q).numpy()
    q = torch.from_numpy(folded.view(np.int16).copy()).view(tdt)
    if average:
        q.div_(N)
    return q.to(torch.float32).numpy()


@pytest.mark.parametrize("where,average", [("device", True), ("device", False), ("host", True)])
def test_bf16_push_pull_matches_the_host(where, average):
    from prophet_amd.pushpull import ServerFrontend, Worker
    from prophet_amd.server import PSServer
    assert torch.cuda.is_available()
    srv = PSServer(N)
    fe = ServerFrontend(srv)
    workers = [Worker(r, fe, partition_bytes=64 << 10) for r in range(N)]
    data = {(r, it): _grad(r, it) for r in range(N) for it in range(ITERS + 1)}
    put = (lambda a: torch.from_numpy(a).cuda()) if where == "device" else (lambda a: a.copy())
    held = {k: put(v) for k, v in data.items()}
    bar = threading.Barrier(N + 1)
    errors = []

    def run(w):
        try:
            w.declare("g")
            ctx = w.init_tensor("g", held[(w.rank, 0)], DType.FLOAT32,
                                compression=Compression.bf16)
            assert ctx.dtype == DType.BFLOAT16 and ctx.size == 2 * NELEM
            for it in range(1, ITERS + 1):
                w.push_pull("g", held[(w.rank, it)], average=average)       # in place
                if where == "device":
                    torch.cuda.current_stream().synchronize()
                bar.wait(timeout=60)             # main thread reads arrival orders
                bar.wait(timeout=60)
        except Exception as e:  # surfaced below
            errors.append(repr(e))
            bar.abort()

    ts = [threading.Thread(target=run, args=(w,)) for w in workers]
    for t in ts:
        t.start()
    port = PortReducer(nthreads=4)
    try:
        for it in range(1, ITERS + 1):
            bar.wait(timeout=120)
            parts = workers[0].contexts["g"].parts
            assert [ln for _, _, ln in parts] == [65536, 65536, 2 * 4097]
            orders = {key: srv.key_info(key)[2] for key, _, _ in parts}
            got = {r: (held[(r, it)].cpu().numpy() if where == "device" else held[(r, it)])
                   for r in range(N)}
            bar.wait(timeout=60)
            xs = [data[(r, it)] for r in range(N)]
            for key, off, ln in parts:
                order = orders[key]
                assert sorted(order) == list(range(N))
                want = _expected(port, xs, order, off, ln, "bf16", average)
                assert not np.isnan(want).any()
                if key == parts[0][0]:
                    # the feature: finite where the fp16 wire gives inf
                    assert np.isfinite(want[:32]).all() and (np.abs(want[:32]) > 2e4).all()
                    fp16 = _expected(port, xs, order, off, ln, "fp16", average)
                    assert np.isinf(fp16[:32]).all()
                    assert (want[48:80] != 0).all() and (np.abs(want[48:80]) < 2.0 ** -126).all()
                for r in range(N):
                    g = got[r][off // 2:(off + ln) // 2]
                    assert np.isfinite(g[:32]).all()
                    assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (it, key, r)
    except threading.BrokenBarrierError:
        pass                                     # a worker failed: reported below
    except BaseException:
        bar.abort()                              # let the workers go, then fail
        raise
    for t in ts:
        t.join(timeout=60)
    assert not errors, errors
    srv.close()


def test_one_iteration_mixes_none_fp16_and_bf16():
    from prophet_amd.pushpull import ServerFrontend, Worker
    from prophet_amd.server import PSServer
    assert torch.cuda.is_available()
    names = ["n", "h", "b"]                      # declared in this order
    comp = {"n": Compression.none, "h": Compression.fp16, "b": Compression.bf16}
    wire = {"n": "none", "h": "fp16", "b": "bf16"}
    srv = PSServer(N)
    fe = ServerFrontend(srv)
    workers = [Worker(r, fe, partition_bytes=64 << 10) for r in range(N)]
    data = {(r, it, nm): _grad(r, 10 * it + i) for r in range(N) for it in range(ITERS + 1)
            for i, nm in enumerate(names)}
    held = {r: {nm: torch.from_numpy(data[(r, 1, nm)]).cuda() for nm in names} for r in range(N)}
    bar = threading.Barrier(N + 1)
    errors, built = [], {}

    def run(w):
        try:
            for nm in names:
                w.declare(nm)
            for nm in names:
                ctx = w.init_tensor(nm, torch.from_numpy(data[(w.rank, 0, nm)]).cuda(),
                                    DType.FLOAT32, compression=comp[nm])
                assert ctx.dtype == WIRE[wire[nm]][0]
            for it in range(1, ITERS + 1):
                if it > 1:
                    for nm in names:
                        held[w.rank][nm].copy_(torch.from_numpy(data[(w.rank, it, nm)]))
                w.push_pull_iteration(held[w.rank], average=True)
                torch.cuda.current_stream().synchronize()
                built[(w.rank, it)] = (w._cast_plans.built, len(w._cast_plans))
                bar.wait(timeout=60)
                bar.wait(timeout=60)
        except Exception as e:  # surfaced below
            errors.append(repr(e))
            bar.abort()

    ts = [threading.Thread(target=run, args=(w,)) for w in workers]
    for t in ts:
        t.start()
    port = PortReducer(nthreads=4)
    try:
        for it in range(1, ITERS + 1):
            bar.wait(timeout=120)
            ctxs = workers[0].contexts
            orders = {key: srv.key_info(key)[2] for nm in names for key, _, _ in ctxs[nm].parts}
            got = {r: {nm: held[r][nm].cpu().numpy() for nm in names} for r in range(N)}
            bar.wait(timeout=60)
            for nm in names:
                xs = [data[(r, it, nm)] for r in range(N)]
                es = 4 if nm == "n" else 2
                for key, off, ln in ctxs[nm].parts:
                    want = _expected(port, xs, orders[key], off, ln, wire[nm], True)
                    assert not np.isnan(want).any()
                    if off == 0:
                        assert np.isinf(want[:32]).all() == (nm == "h")
                    for r in range(N):
                        g = got[r][nm][off // es:(off + ln) // es]
                        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), \
                            (it, nm, key, r)
    except threading.BrokenBarrierError:
        pass
    except BaseException:
        bar.abort()
        raise
    for t in ts:
        t.join(timeout=60)
    assert not errors, errors
    for r in range(N):
        # one plan per compressed group, built in the first iteration and found again
        assert built[(r, 1)] == (2, 2) and built[(r, 2)] == (2, 2), built
    for w in workers:
        w.close()
    srv.close()
