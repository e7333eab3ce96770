"""``push_pull_iteration(..., clip_norm=, unscale=)`` over the real GPU-resident
server: two workers, device tensors, one iteration mixing an
``fp16`` tensor, a ``bf16_ef`` tensor, an uncompressed f32 tensor and an int32
tensor, ``average=True``, ``clip_norm`` below the true norm, ``unscale=2**-7``.

Every floating output equals ``mult`` times what the same iteration gives
without ``clip_norm`` — the f32 product, one rounding, bit for bit;
``grad_clip.norm`` is the f64 norm of those unclipped outputs times the
unscale, within the any-order bound of the sum of squares (``N * 2**-52``
relative over N elements, half of it after the square root) plus the record's
own ``4 * 2**-52``; the f64 norm of the clipped outputs lies within ``2**-23``
relative of ``coef * norm`` (each product rounds once in f32, and so does
``mult``); the int tensor keeps the sum it pulled and is named in ``skipped``;
``grad_clip``'s fields are 0-d device tensors; the second iteration reuses the
cached plans; one injected inf gives ``found_inf == 1`` and a finite norm."""
import threading

import numpy as np
import pytest

from prophet_amd.compression import Compression
from prophet_amd.dtypes import DType

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

NAMES = ["a16", "bef", "plain", "ints"]
FLOATS = NAMES[:3]
COMPS = [Compression.fp16, Compression.bf16_ef, Compression.none, Compression.none]
SIZES = [4099, 2 * 2048 + 13, 3000, 515]
ITERS = 3                                   # the last one carries an inf
HOT = 5
UNSCALE = 2.0 ** -7
CLIP = 1.0


def _grad(rank, it, i):
    rng = np.random.default_rng(100 * it + 10 * rank + i)
    if NAMES[i] == "ints":
        return rng.integers(-1000, 1000, SIZES[i]).astype(np.int32)
    x = (rng.standard_normal(SIZES[i]) * np.exp2(rng.integers(-6, 6, SIZES[i]))).astype(np.float32)
    if NAMES[i] == "a16" and it == ITERS and rank == 1:
        x[HOT] = np.inf
    return x


def _rounds(clip):
    """ITERS iterations of two workers over a fresh server; per (rank, it) the
    outputs on the host and what the worker left behind."""
    from prophet_amd.pushpull import ServerFrontend, Worker
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
                dt = DType.INT32 if nm == "ints" else DType.FLOAT32
                w.init_tensor(nm, torch.from_numpy(_grad(w.rank, 0, i)).cuda(), dt,
                              compression=comp)
            held = {nm: torch.from_numpy(_grad(w.rank, 0, i)).cuda()
                    for i, nm in enumerate(NAMES)}
            for it in range(1, ITERS + 1):
                for i, nm in enumerate(NAMES):
                    held[nm].copy_(torch.from_numpy(_grad(w.rank, it, i)))
                clipped = None
                if clip:
                    unscale = UNSCALE if it == 1 else \
                        torch.tensor([UNSCALE], dtype=torch.float32, device="cuda")
                    w.push_pull_iteration(held, average=True, clip_norm=CLIP, unscale=unscale)
                    gc = w.grad_clip
                    # device tensors, in stream order, before any sync
                    fields = (gc.norm, gc.coef, gc.mult, gc.found_inf, gc.sumsq)
                    assert all(t.is_cuda and t.dim() == 0 for t in fields) and gc.rows.is_cuda
                    skip = torch.where(gc.found_inf > 0, 1, 0)          # usable on the device
                    clipped = (gc, fields, skip, w.grad_stats)
                else:
                    # the same rounds without the clip: the floats averaged,
                    # the ints (no average for integers) on their own
                    w.push_pull_iteration({nm: held[nm] for nm in FLOATS}, average=True)
                    w.push_pull("ints", held["ints"])
                torch.cuda.current_stream().synchronize()
                if clipped is not None:
                    gc, fields, skip, gs = clipped
                    clipped = (gc.names, gc.skipped, [float(t) for t in fields], int(skip),
                               gc.rows.cpu().numpy().copy(), gs.names, gs.skipped,
                               gs.rows.cpu().numpy().copy())
                seen[(w.rank, it)] = ({nm: held[nm].cpu().numpy().copy() for nm in NAMES},
                                      clipped, w._cast_plans.built)
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


def _finite_sumsq(x):
    v = x.astype(np.float64)
    fin = np.isfinite(v)
    return float(np.square(v[fin]).sum()), int(np.count_nonzero(~fin))


def test_outputs_are_mult_times_the_unclipped_outputs(rounds):
    for key, (outs, clipped, _) in sorted(rounds[True].items()):
        ref = rounds[False][key][0]
        mult = np.float32(clipped[2][2])
        for nm in FLOATS:
            want = ref[nm] * mult                                # f32 product, one rounding
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(outs[nm]), nan), (key, nm)
            assert np.array_equal(outs[nm].view(np.uint32)[~nan], want.view(np.uint32)[~nan]), \
                (key, nm)
        # the int tensor keeps the sum it pulled: neither divided nor multiplied
        assert np.array_equal(outs["ints"], ref["ints"])
        rank, it = key
        assert np.array_equal(outs["ints"], _grad(0, it, 3) + _grad(1, it, 3))


def test_record_matches_the_unclipped_outputs(rounds):
    n_total = sum(SIZES[:3])
    for key, (outs, clipped, _) in sorted(rounds[True].items()):
        ref = rounds[False][key][0]
        names, skipped, (norm, coef, mult, found_inf, sumsq), skip, rows, gn, gsk, grows = clipped
        assert names == ["a16", "bef", "plain"] and skipped == ["ints"]
        assert gn == ["a16", "bef"] and gsk == ["plain", "ints"]     # as stats=True would
        assert np.array_equal(grows, rows[:2])
        ss, nf = zip(*(_finite_sumsq(ref[nm]) for nm in FLOATS))
        assert rows[:, 1].tolist() == list(map(float, nf)) and found_inf == float(sum(nf))
        for i, nm in enumerate(FLOATS):
            assert abs(rows[i, 0] - ss[i]) <= ref[nm].size * 2.0 ** -52 * ss[i], (key, nm)
        norm_ref = float(np.sqrt(sum(ss))) * UNSCALE
        print(f"{key}: norm {norm!r} ref {norm_ref!r} coef {coef!r} mult {mult!r} "
              f"found_inf {found_inf}")
        assert abs(norm - norm_ref) <= (n_total * 2.0 ** -53 + 4 * 2.0 ** -52) * norm_ref
        assert norm > CLIP and coef < 1.0                           # the clip bites
        assert abs(coef - CLIP / (norm + 1e-6)) <= np.spacing(np.float32(coef))
        assert mult == coef * UNSCALE                                # a power of two: exact
        # the clipped outputs' norm: each product rounds once in f32
        after = float(np.sqrt(sum(_finite_sumsq(outs[nm])[0] for nm in FLOATS)))
        assert abs(after - coef * norm) <= 2.0 ** -23 * coef * norm, (key, after, coef * norm)
        assert after <= CLIP * (1 + 2.0 ** -22)


def test_an_injected_inf_is_found_and_the_norm_stays_finite(rounds):
    for rank in range(2):
        for it in range(1, ITERS + 1):
            outs, clipped, _ = rounds[True][(rank, it)]
            norm, found_inf, skip = clipped[2][0], clipped[2][3], clipped[3]
            assert np.isfinite(norm)
            assert found_inf == (1.0 if it == ITERS else 0.0) and skip == int(it == ITERS)
        assert np.isinf(rounds[True][(rank, ITERS)][0]["a16"][HOT])   # inf stays inf


def test_cached_plans_are_reused(rounds):
    for rank in range(2):
        # fp16 and bf16_ef: one plan each, built in the first iteration, serving
        # the compress, the measure and the scaled decompress
        assert [rounds[True][(rank, it)][2] for it in range(1, ITERS + 1)] == [2] * ITERS
