"""``push_pull_iteration(..., apply=SgdStep(...))`` over the real GPU-resident
server: two workers on one in-process server, four device
tensors of 1, 8, 5,000 and 70,001 float32 elements under ``fp16``, ``bf16``,
``fp16_ef`` and ``bf16_sr``, ``average=True``; once with ``apply`` alone and
once with ``clip_norm``, ``unscale`` (a 1-element device tensor) and
``skip_nonfinite``.

After every iteration the parameters and ``Worker.momentum`` equal
``prophet_amd.sgd.sgd_step`` applied on the host to the previous parameters
and momenta, the context's staging buffer (the pulled wire aggregate, still
there) and the record's ``mult`` read back, bit for bit; both workers hold
identical parameters; the gradients in ``tensors`` keep their bytes; the
second iteration continues from the first one's momenta; an inf pushed by one
worker makes ``grad_clip.found_inf`` non-zero and leaves every byte of the
parameters and momenta; the ``ValueError``s are raised before anything is
pushed."""
import threading

import numpy as np
import pytest

from prophet_amd import sgd
from prophet_amd.compression import Compression
from prophet_amd.dtypes import DType

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

NAMES = ["one", "eight", "mid", "big"]
SIZES = [1, 8, 5000, 70001]
COMPS = [Compression.fp16, Compression.bf16, Compression.fp16_ef, Compression.bf16_sr]
WIRES = ["fp16", "bf16", "fp16", "bf16"]
ITERS = 3                                   # with the clip, the last one carries an inf
HOT = 4321
UNSCALE = 2.0 ** -7
CLIP = 1.0
HYPER = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)


def _grad(rank, it, i, clip):
    rng = np.random.default_rng(100 * it + 10 * rank + i)
    x = (rng.standard_normal(SIZES[i]) * np.exp2(rng.integers(-6, 6, SIZES[i]))).astype(np.float32)
    if clip and NAMES[i] == "mid" and it == ITERS and rank == 1:
        x[HOT] = np.inf
    return x


def _param(i):
    rng = np.random.default_rng(7 + i)
    return (rng.standard_normal(SIZES[i]) * np.exp2(rng.integers(-8, 4, SIZES[i]))).astype(
        np.float32)


def _host(t):
    return t.detach().cpu().numpy().copy()


def _wire_bits(t):
    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16).copy()


def _rounds(clip):
    """ITERS iterations of two workers over a fresh server; per (rank, it)
    what the worker holds afterwards, on the host."""
    from prophet_amd.pushpull import ServerFrontend, SgdStep, Worker
    from prophet_amd.server import PSServer
    srv = PSServer(2)
    fe = ServerFrontend(srv)
    workers = [Worker(r, fe) for r in range(2)]
    seen, errors = {}, []

    def run(w):
        try:
            for nm in NAMES:
                w.declare(nm)
            for i, (nm, comp) in enumerate(zip(NAMES, COMPS)):
                w.init_tensor(nm, torch.from_numpy(_grad(w.rank, 0, i, clip)).cuda(),
                              DType.FLOAT32, compression=comp)
            held = {nm: torch.from_numpy(_grad(w.rank, 0, i, clip)).cuda()
                    for i, nm in enumerate(NAMES)}
            params = {nm: torch.from_numpy(_param(i)).cuda() for i, nm in enumerate(NAMES)}
            step = SgdStep(params, skip_nonfinite=clip, **HYPER)
            assert all(w.momentum(nm) is None for nm in NAMES)
            # the errors come before anything is pushed: one worker alone may raise them
            bad = [SgdStep({**params, "big": params["big"].cpu()}, lr=0.1),        # place
                   SgdStep({**params, "big": params["big"][:-1]}, lr=0.1),          # size
                   SgdStep({k: v for k, v in params.items() if k != "mid"}, lr=0.1),
                   SgdStep(params, lr=0.1, skip_nonfinite=True),            # no clip_norm
                   SgdStep(params, lr=0.1, momentum=1.0)]
            for b in bad:
                with pytest.raises(ValueError):
                    w.push_pull_iteration(held, average=True, apply=b)
            for it in range(1, ITERS + 1):
                for i, nm in enumerate(NAMES):
                    held[nm].copy_(torch.from_numpy(_grad(w.rank, it, i, clip)))
                kw = {}
                if clip:
                    kw = dict(clip_norm=CLIP,
                              unscale=torch.tensor([UNSCALE], dtype=torch.float32, device="cuda"))
                w.push_pull_iteration(held, average=True, apply=step, **kw)
                rec = None
                if clip:
                    gc = w.grad_clip
                    assert gc.found_inf.is_cuda and gc.mult.is_cuda       # no host round trip
                    rec = gc
                torch.cuda.current_stream().synchronize()
                seen[(w.rank, it)] = dict(
                    grads={nm: _host(held[nm]) for nm in NAMES},
                    params={nm: _host(params[nm]) for nm in NAMES},
                    momenta={nm: _host(w.momentum(nm)) for nm in NAMES},
                    wire={nm: _wire_bits(w.contexts[nm].staging) for nm in NAMES},
                    mult=None if rec is None else np.float32(float(rec.mult)),
                    found_inf=None if rec is None else float(rec.found_inf),
                    names=None if rec is None else (rec.names, rec.skipped),
                    built=w._cast_plans.built)
        except Exception as e:              # noqa: BLE001 — surfaced below
            import traceback
            errors.append(traceback.format_exc() or repr(e))

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
    return {flag: _rounds(flag) for flag in (False, True)}


def _same(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.parametrize("clip", [False, True], ids=["apply", "apply+clip"])
def test_parameters_and_momenta_are_the_definition(rounds, clip):
    for rank in range(2):
        p = {nm: _param(i) for i, nm in enumerate(NAMES)}
        m = {nm: np.zeros(n, np.float32) for nm, n in zip(NAMES, SIZES)}
        for it in range(1, ITERS + 1):
            got = rounds[clip][(rank, it)]
            skipped = clip and got["found_inf"] != 0
            for nm, wire in zip(NAMES, WIRES):
                if not skipped:
                    p[nm], m[nm] = sgd.sgd_step(p[nm], m[nm], got["wire"][nm], wire, 2,
                                                mult=got["mult"], **HYPER)
                assert _same(got["params"][nm], p[nm]), (clip, rank, it, nm)
                assert _same(got["momenta"][nm], m[nm]), (clip, rank, it, nm)
                # the gradients keep their bytes
                i = NAMES.index(nm)
                assert np.array_equal(got["grads"][nm].view(np.uint32),
                                      _grad(rank, it, i, clip).view(np.uint32)), (rank, it, nm)
    # a step moved the parameters at all, and the momenta left zero
    last = rounds[clip][(0, 2)]
    assert not np.array_equal(last["params"]["big"], _param(3))
    assert np.count_nonzero(last["momenta"]["big"]) > SIZES[3] // 2


@pytest.mark.parametrize("clip", [False, True], ids=["apply", "apply+clip"])
def test_both_workers_hold_identical_parameters(rounds, clip):
    for it in range(1, ITERS + 1):
        a, b = rounds[clip][(0, it)], rounds[clip][(1, it)]
        for nm in NAMES:
            assert np.array_equal(a["wire"][nm], b["wire"][nm]), (it, nm)
            assert np.array_equal(a["params"][nm].view(np.uint32),
                                  b["params"][nm].view(np.uint32)), (it, nm)
            assert np.array_equal(a["momenta"][nm].view(np.uint32),
                                  b["momenta"][nm].view(np.uint32)), (it, nm)


def test_an_injected_inf_skips_the_step_on_the_device(rounds):
    for rank in range(2):
        before, after = rounds[True][(rank, ITERS - 1)], rounds[True][(rank, ITERS)]
        assert before["found_inf"] == 0.0 and after["found_inf"] == 1.0
        assert after["names"] == (NAMES, [])
        for nm in NAMES:
            assert np.array_equal(after["params"][nm].view(np.uint32),
                                  before["params"][nm].view(np.uint32)), nm
            assert np.array_equal(after["momenta"][nm].view(np.uint32),
                                  before["momenta"][nm].view(np.uint32)), nm
        assert 0 < float(before["mult"]) < UNSCALE, "the clip bites"
        # without the clip (no inf injected) the third step is applied
        plain2, plain3 = rounds[False][(rank, ITERS - 1)], rounds[False][(rank, ITERS)]
        assert not np.array_equal(plain3["params"]["big"], plain2["params"]["big"])


def test_cached_plans_are_reused(rounds):
    for clip in (False, True):
        for rank in range(2):
            # per compressor the compress (and measure) plan and the SGD plan,
            # all built in the first iteration
            assert [rounds[clip][(rank, it)]["built"] for it in range(1, ITERS + 1)] == [8] * ITERS
