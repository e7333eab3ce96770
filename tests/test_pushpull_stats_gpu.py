"""``push_pull_iteration(..., stats=True)`` over the real GPU-resident server,
two workers, f32 device tensors, one iteration mixing ``Compression.none``,
``fp16``, ``bf16_ef`` and ``fp16_sr`` with ``average=True``:
``Worker.grad_stats`` holds one row per compressed context — the definition
(``compression.decompress_stats``) applied to the outputs, the counts exact,
the sums within the any-order bound ``nelem * 2**-52 * ref`` — names the
uncompressed context in ``.skipped``, reports the one inf that two pushed
values of 40,000 sum to on the fp16 wire, stays on the device, reuses the
cached plans on the second iteration, and the outputs are bit for bit those of
the same rounds run with ``stats=False``."""
import threading

import numpy as np
import pytest

from prophet_amd.compression import Compression, decompress_stats
from prophet_amd.dtypes import DType

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

NAMES = ["plain", "a16", "bef", "sr16"]
COMPS = [Compression.none, Compression.fp16, Compression.bf16_ef, Compression.fp16_sr]
SIZES = [3000, 4099, 2 * 2048 + 13, 777]
ITERS = 2
HOT = 5                                     # a16[HOT] is 40,000 on both workers


def _grad(rank, it, i):
    rng = np.random.default_rng(100 * it + 10 * rank + i)
    x = (rng.standard_normal(SIZES[i]) * np.exp2(rng.integers(-6, 6, SIZES[i]))).astype(np.float32)
    if NAMES[i] == "a16":
        x[HOT] = 40000.0
    return x


def _rounds(stats):
    """ITERS iterations of two workers over a fresh server; per (rank, it) the
    outputs on the host, the GradStats and the plans built so far."""
    from prophet_amd.pushpull import ServerFrontend, Worker
    from prophet_amd.server import PSServer
    srv = PSServer(2)
    fe = ServerFrontend(srv)
    workers = [Worker(r, fe, sr_seed=3) for r in range(2)]
    seen, errors = {}, []

    def run(w):
        try:
            for nm in NAMES:
                w.declare(nm)
            for i, (nm, comp) in enumerate(zip(NAMES, COMPS)):
                w.init_tensor(nm, torch.from_numpy(_grad(w.rank, 0, i)).cuda(), DType.FLOAT32,
                              compression=comp)
            held = {nm: torch.empty(n, device="cuda") for nm, n in zip(NAMES, SIZES)}
            for it in range(1, ITERS + 1):
                for i, nm in enumerate(NAMES):
                    held[nm].copy_(torch.from_numpy(_grad(w.rank, it, i)))
                w.push_pull_iteration(held, average=True, stats=stats)
                gs = w.grad_stats
                dev = None
                if stats:
                    # derived on the device, in stream order, before any sync
                    dev = (gs.sumsq(), gs.nonfinite(), gs.norm(), gs["a16"])
                    assert all(t.is_cuda for t in dev) and gs.rows.is_cuda
                    assert dev[0].dim() == 0 and dev[1].dim() == 0 and dev[2].dim() == 0
                torch.cuda.current_stream().synchronize()
                seen[(w.rank, it)] = ({nm: held[nm].cpu().numpy().copy() for nm in NAMES},
                                      gs, None if dev is None else [t.cpu() for t in dev],
                                      None if gs is None else gs.rows.cpu().numpy().copy(),
                                      w._cast_plans.built)
        except Exception as e:              # noqa: BLE001 — surfaced below
            errors.append(repr(e))

    ts = [threading.Thread(target=run, args=(w,), name=f"w{w.rank}") for w in workers]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
    assert not errors, errors
    for w in workers:
        w.close()
    srv.close()
    return seen


@pytest.fixture(scope="module")
def rounds():
    assert torch.cuda.is_available()
    return {flag: _rounds(flag) for flag in (True, False)}


def test_rows_are_the_definition_of_the_outputs(rounds):
    for (rank, it), (outs, gs, dev, rows, built) in sorted(rounds[True].items()):
        assert gs.names == ["a16", "bef", "sr16"] and gs.skipped == ["plain"]
        assert rows.shape == (3, 2) and rows.dtype == np.float64
        total, bad = 0.0, 0
        for i, nm in enumerate(gs.names):
            ss, nf = decompress_stats(outs[nm])
            n = outs[nm].size
            print(f"rank {rank} it {it} {nm}: sumsq {rows[i, 0]!r} ref {ss!r} "
                  f"nonfinite {rows[i, 1]} ref {nf}")
            assert rows[i, 1] == nf, (rank, it, nm)
            assert abs(rows[i, 0] - ss) <= n * 2.0 ** -52 * ss, (rank, it, nm)
            total, bad = total + ss, bad + nf
        # two pushed values of 40,000 sum to inf on the fp16 wire
        assert np.isinf(outs["a16"][HOT]) and rows[0, 1] == 1 and bad == 1
        assert float(dev[1]) == 1.0 and dev[3].tolist() == rows[0].tolist()
        assert float(dev[0]) == pytest.approx(total, rel=1e-12)
        assert float(dev[2]) == pytest.approx(total ** 0.5, rel=1e-12)


def test_cached_plans_are_reused(rounds):
    for flag in (True, False):
        for rank in range(2):
            # fp16, bf16_ef, fp16_sr: one plan each, built in the first iteration
            assert rounds[flag][(rank, 1)][4] == 3
            assert rounds[flag][(rank, 2)][4] == 3


def test_outputs_equal_a_run_without_statistics(rounds):
    assert rounds[False][(0, 1)][1] is None                  # no GradStats without stats=True
    for key, (outs, *_) in rounds[True].items():
        for nm in NAMES:
            assert np.array_equal(outs[nm].view(np.uint32),
                                  rounds[False][key][0][nm].view(np.uint32)), (key, nm)
    # both workers were delivered the same aggregate
    for it in range(1, ITERS + 1):
        for nm in ("plain", "a16", "bef"):
            assert np.array_equal(rounds[True][(0, it)][0][nm].view(np.uint32),
                                  rounds[True][(1, it)][0][nm].view(np.uint32))
