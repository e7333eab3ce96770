"""push_pull with ``Compression.fp16_sr`` / ``bf16_sr`` over the real
GPU-resident server, one worker (its "sum" is what it pushed), f32 device
tensors: a constant gradient the plain wire never delivers — 1e-8 on fp16,
the 2^-12 of 1 + 2^-12 on bf16 — arrives in expectation, and every round's
result is bit-equal to the same rounds run on host tensors, which go through
the numpy definition (prophet_amd/sr.py).  A ``push_pull_iteration`` over a
mixed set on the device equals the same iteration on the host, and its plans
are built once."""
import numpy as np
import pytest

from prophet_amd import sr
from prophet_amd.compression import Compression
from prophet_amd.dtypes import DType

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

NELEM, ROUNDS, SEED = 1 << 16, 64, 2026


class LastPushServer:
    """One worker's host server: a pull returns the key's last push."""

    def __init__(self):
        self.store = {}

    def push(self, key, worker, data, dtype, nbytes=None):
        self.store[key] = np.asarray(data).view(np.uint8).copy()

    def pull(self, key, out, nbytes=None):
        np.asarray(out).view(np.uint8)[:] = self.store[key]


CASES = {"fp16": (Compression.fp16_sr, Compression.fp16, DType.FLOAT16, np.float32(1e-8)),
         "bf16": (Compression.bf16_sr, Compression.bf16, DType.BFLOAT16,
                  np.float32(1 + 2.0 ** -12))}


@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_constant_gradient_arrives_and_matches_the_host(wire):
    from prophet_amd.pushpull import ServerFrontend, Worker
    from prophet_amd.server import PSServer
    assert torch.cuda.is_available()
    comp, plain, wd, g = CASES[wire]
    srv = PSServer(1)
    dev = Worker(0, ServerFrontend(srv), sr_seed=SEED)
    host = Worker(0, ServerFrontend(LastPushServer(), size=1), sr_seed=SEED)
    for w in (dev, host):
        w.declare("g")
    x0 = np.full(NELEM, g, np.float32)
    ctx = dev.init_tensor("g", torch.from_numpy(x0).cuda(), DType.FLOAT32, compression=comp)
    assert ctx.dtype == wd and ctx.size == 2 * NELEM and ctx.staging.is_cuda
    hctx = host.init_tensor("g", x0.copy(), DType.FLOAT32, compression=comp)
    assert ctx.sr_key == hctx.sr_key == sr.context_key(0, 0, SEED)
    xd = torch.empty(NELEM, device="cuda")
    total = torch.zeros(NELEM, dtype=torch.float64, device="cuda")
    bad = torch.zeros((), dtype=torch.int64, device="cuda")
    for it in range(ROUNDS):
        xd.fill_(float(g))
        dev.push_pull("g", xd)
        xh = x0.copy()
        host.push_pull("g", xh)
        bad += (xd.view(torch.int32) != torch.from_numpy(xh.view(np.int32)).cuda()).sum()
        total += xd.double()
    assert dev.sr_step == host.sr_step == ROUNDS
    assert int(bad) == 0                          # bit-equal to the host rounds, every round
    # what the plain wire delivers of the same gradient, every round
    xp = torch.full((NELEM,), float(g), device="cuda")
    xp = plain.decompress(*plain.compress(xp))
    delivered = float(total.sum()) / (NELEM * ROUNDS)
    if wire == "fp16":
        assert float(xp.abs().sum()) == 0.0       # the plain wire: exactly 0, every round
        assert bool((total > 0).any()) and delivered > 0
        step, p = 2.0 ** -24, float(g) / 2.0 ** -24
    else:
        assert bool((xp == 1.0).all())            # the plain wire: exactly 1.0
        assert delivered > 1.0
        step, p = 2.0 ** -7, 2.0 ** -5
    # within 6 standard errors of g under the binomial model
    se = step * np.sqrt(p * (1 - p) / (NELEM * ROUNDS))
    assert abs(delivered - float(g)) <= 6 * se + (2.0 ** -40 if wire == "fp16" else 0)
    with pytest.raises(ValueError):
        dev.broadcast("g", xd, root_rank=0)
    for w in (dev, host):
        w.close()
    srv.close()


def test_iteration_over_a_mixed_set_matches_the_host():
    """none, bf16, bf16_ef, fp16_sr and two bf16_sr contexts in one iteration,
    three times, on the device and on the host: the same bytes (one SR plan
    launch a compressor, every context under its own key, one step each), and
    the device's plans are built in the first iteration only."""
    from prophet_amd.pushpull import ServerFrontend, Worker
    from prophet_amd.server import PSServer
    names = ["n", "b", "be", "hs", "bs", "bs2"]
    comps = [Compression.none, Compression.bf16, Compression.bf16_ef, Compression.fp16_sr,
             Compression.bf16_sr, Compression.bf16_sr]
    sizes = [4099, 2048 * 3 + 5, 777, 2048 * 2 + 13, 9, 2048 * 5 + 1]
    rng = np.random.default_rng(61)
    data = {(nm, it): (rng.standard_normal(n) * np.exp2(rng.integers(-30, 10, n)))
            .astype(np.float32) for nm, n in zip(names, sizes) for it in range(4)}
    srv = PSServer(1)
    dev = Worker(0, ServerFrontend(srv), sr_seed=7)
    host = Worker(0, ServerFrontend(LastPushServer(), size=1), sr_seed=7)
    for w in (dev, host):
        for nm in names:
            w.declare(nm)
    for nm, comp in zip(names, comps):
        dev.init_tensor(nm, torch.from_numpy(data[(nm, 0)]).cuda(), DType.FLOAT32,
                        compression=comp)
        host.init_tensor(nm, data[(nm, 0)].copy(), DType.FLOAT32, compression=comp)
    held = {nm: torch.empty(n, device="cuda") for nm, n in zip(names, sizes)}
    for it in range(1, 4):
        for nm in names:
            held[nm].copy_(torch.from_numpy(data[(nm, it)]))
        xh = {nm: data[(nm, it)].copy() for nm in names}
        dev.push_pull_iteration(held)
        host.push_pull_iteration(xh)
        torch.cuda.current_stream().synchronize()
        for nm in names:
            assert np.array_equal(held[nm].cpu().numpy().view(np.uint32),
                                  xh[nm].view(np.uint32)), (it, nm)
        assert dev.sr_step == host.sr_step == 2 * it
        # bf16, bf16_ef, fp16_sr, bf16_sr: one plan each, built in the first iteration
        assert (dev._cast_plans.built, len(dev._cast_plans)) == (4, 4)
    assert np.array_equal(dev.residual("be").cpu().numpy().view(np.uint32),
                          host.residual("be").view(np.uint32))
    # what the SR contexts pulled is not what the plain cast would have given
    for nm, comp in (("hs", Compression.fp16), ("bs2", Compression.bf16)):
        plain, ctx = comp.compress(torch.from_numpy(data[(nm, 3)]))
        assert not torch.equal(comp.decompress(plain, ctx), held[nm].cpu())
    for w in (dev, host):
        w.close()
    srv.close()
