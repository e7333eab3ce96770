"""push_pull with ``Compression.fp16`` over the real GPU-resident server: 3
worker threads, f32 tensors travelling as fp16 (three partitions, the last
odd-sized), folded by the server's fp16 kernel, averaged on the fp16 value and
widened by one fused launch.  Every worker's every bit equals the host's
``widen(div_f16(fold_f16(compress(x_r))))`` in the server's recorded arrival
order: CPU torch casts and ``div_``, the oracle's fp16 fold."""
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


def _grad(rank, it):
    rng = np.random.default_rng(100 * it + rank)
    x = (rng.standard_normal(NELEM) * np.exp2(rng.integers(-4, 12, NELEM))).astype(np.float32)
    # past fp16's range (one sign per index on every worker: no inf - inf, so
    # no NaN), and inside its subnormal range
    x[0:16] = 7e4 + rank
    x[16:32] = -(65520.0 + 100 * rank)
    x[32:48] = 65519.0 - rank
    x[48:64] = (np.arange(16) + 1 + rank) * np.float32(2.0 ** -25)
    x[64:80] = -(np.arange(16) + 3 * rank) * np.float32(3e-8)
    x[80:84] = [0.0, -0.0, 6.1e-5, -6.0e-5]
    return x


@pytest.mark.parametrize("where,average", [("device", True), ("device", False), ("host", True)])
def test_compressed_push_pull_matches_the_host(where, average):
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
                                compression=Compression.fp16)
            assert ctx.dtype == DType.FLOAT16 and ctx.size == 2 * NELEM
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
            halves = {r: torch.from_numpy(data[(r, it)]).to(torch.float16).numpy().view(np.uint8)
                      for r in range(N)}
            for key, off, ln in parts:
                order = orders[key]
                assert sorted(order) == list(range(N))
                folded = np.zeros(ln, np.uint8)
                assert port.sum_n(folded, [halves[r][off:off + ln].copy() for r in order], ln,
                                  DType.FLOAT16) == 0
                q = torch.from_numpy(folded.view(np.float16).copy())
                if average:
                    q.div_(N)
                want = q.to(torch.float32).numpy()
                assert not np.isnan(want).any()
                if key == parts[0][0]:
                    assert np.isinf(want[:32]).all() and (want[48:64] != 0).any()
                for r in range(N):
                    g = got[r][off // 2:(off + ln) // 2]
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
