"""Stochastic-rounding cast plans (byteps_reduce_cast_plan_create_sr /
_compress_sr, cast_plan_kernel of prophet_amd/csrc/bpsr_cast_plan.h under the
scheme of bpsr_cast_sr.h) on the
GPU: one launch over segments of mixed lengths, alignments and keys writes per
segment the bytes of one ``compress_sr`` — and so of the host definition
(prophet_amd/sr.py) — the plan's decompress is the plain one, a compress
without a step is refused, and the plan cache's key carries the keys."""
import numpy as np
import pytest

from prophet_amd import reducer, sr
from prophet_amd.compression import CastPlanCache, Compression
from prophet_amd.dtypes import DType
from prophet_amd.reducer import GpuReducer, SrKey

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

F32 = DType.FLOAT32
WIRES = [(DType.FLOAT16, torch.float16, "fp16"), (DType.BFLOAT16, torch.bfloat16, "bf16")]
IDS = ["fp16", "bf16"]
TILE = 256 * 8
# (elements, wide offset in elements, wire offset in elements); the two sides
# co-align iff the offsets agree mod 4, after a head of (8 - wire offset) % 8.
# Empty, one element, a tile - 1 / exactly / + 1, heads of 3, 2, 1 and 5 (no
# multiple of 4: every vector straddles two Philox groups), sides that never
# co-align (short, and long enough for several element records), several tiles
SEGS = [(0, 0, 0), (1, 0, 0), (TILE - 1, 0, 0), (TILE, 0, 0), (TILE + 1, 0, 0),
        (TILE + 20, 1, 5), (TILE + 20, 2, 6), (TILE + 20, 3, 7), (3 * TILE + 13, 3, 3),
        (777, 0, 1), (5, 2, 2), (5 * TILE + 9, 1, 3)]
KEYS = [0x9e3779b9 * (i + 1) & 0xffffffff for i in range(len(SEGS))]


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return GpuReducer(device=0)


def _aligned(nelem, dtype, off):
    """A device tensor of `nelem` elements `off` elements past a 256-byte boundary."""
    es = torch.empty(0, dtype=dtype).element_size()
    raw = torch.empty((nelem + off) * es + 256, dtype=torch.uint8, device="cuda")
    skip = (-raw.data_ptr()) % 256 + off * es
    return raw[skip:skip + nelem * es].view(dtype)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def grads():
    rng = np.random.default_rng(51)
    out = []
    for n, _, _ in SEGS:
        out.append((rng.standard_normal(n) * np.exp2(rng.integers(-40, 18, n))).astype(np.float32))
    return out


@pytest.mark.parametrize("wd,wt,name", WIRES, ids=IDS)
def test_plan_bytes_are_one_compress_sr_per_segment(red, grads, wd, wt, name):
    assert len(SEGS) == 12 and len(set(KEYS)) == 12
    wides, wires, singles = [], [], []
    for (n, wo, ho), g in zip(SEGS, grads):
        w = _aligned(n, torch.float32, wo)
        w.copy_(torch.from_numpy(g))
        wides.append(w)
        wires.append(_aligned(n, wt, ho))
        singles.append(_aligned(n, wt, ho))
    plan = red.cast_plan([(w, h, w.numel(), SrKey(k)) for w, h, k in zip(wides, wires, KEYS)],
                         F32, wd)
    assert plan.stochastic and not plan.error_feedback
    for step in (0, 0xffffffff):
        for h in wires:
            h.view(torch.int16).fill_(0x5a5a)
        plan.compress(step=step)
        for i, (w, h, s, k, g) in enumerate(zip(wides, wires, singles, KEYS, grads)):
            red.compress_sr(s, w, w.numel(), k, step, wd)
            assert np.array_equal(_bits(h), _bits(s)), (i, step)
            assert np.array_equal(_bits(h), sr.sr_round(g, k, step, name)), (i, step)
    # the plan's decompress is the plain one
    backs = [torch.empty_like(w) for w in wides]
    for w, b in zip(wides, backs):
        b.copy_(w)
        w.fill_(-1.0)
    plan.decompress(2)
    for w, h in zip(wides, wires):
        want = torch.empty_like(w)
        red.decompress(want, h, w.numel(), F32, wd, 2)
        assert torch.equal(w.view(torch.int32), want.view(torch.int32))
    # a compress without a step is refused, and writes nothing
    for h in wires:
        h.view(torch.int16).fill_(0x5a5a)
    with pytest.raises(reducer.ReduceError) as e:
        plan.compress()
    assert e.value.code == reducer.EARGS and "step" in str(e.value)
    torch.cuda.synchronize()
    assert all(bool((h.view(torch.int16) == 0x5a5a).all()) for h in wires)
    plan.close()
    # ... and a step on a plan without keys
    plain = red.cast_plan([(w, h, w.numel()) for w, h in zip(wides, wires)], F32, wd)
    with pytest.raises(reducer.ReduceError) as e:
        plain.compress(step=1)
    assert e.value.code == reducer.EARGS
    plain.close()


def test_empty_plans_and_bad_segments(red):
    e = torch.empty(0, device="cuda")
    eh = torch.empty(0, dtype=torch.bfloat16, device="cuda")
    for segs in ([], [(0, 0, 0, SrKey(1))], [(e, eh, 0, SrKey(1)), (e, eh, 0, SrKey(2))]):
        plan = red.cast_plan(segs, F32, DType.BFLOAT16)
        if segs:
            assert plan.stochastic
            plan.compress(step=3)
            with pytest.raises(reducer.ReduceError):
                plan.compress()                   # an SR plan even when empty
        plan.decompress()
        plan.close()
    wide = torch.zeros(1000, device="cuda")
    wire = torch.zeros(1000, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        red.cast_plan([(wide, wire[:999], 1000, SrKey(1))], F32, DType.BFLOAT16)
    with pytest.raises(reducer.ReduceError) as err:
        red.cast_plan([(wide, wire, 1000, SrKey(1)), (wide[500:], wire[:0], 0, SrKey(2)),
                       (wide[996:], torch.zeros(4, dtype=torch.bfloat16, device="cuda"), 4,
                        SrKey(3))], F32, DType.BFLOAT16)
    assert err.value.code == reducer.EARGS
    with pytest.raises(reducer.ReduceError) as err:
        red.cast_plan([(wide.double(), wire, 1000, SrKey(1))], DType.FLOAT64, DType.BFLOAT16)
    assert err.value.code == reducer.EDTYPE
    torch.cuda.synchronize()


@pytest.mark.parametrize("comp,name", [(Compression.fp16_sr, "fp16"), (Compression.bf16_sr, "bf16")])
def test_compress_many_and_the_cache(comp, name, grads):
    """compress_many_sr_into: one launch, the host definition's bytes; the
    cache hits on the same keys and misses on another key or on the plain plan
    over the same tensors; the SR plan found by its keys also decompresses."""
    idx = [3, 5, 8, 9]
    xs = [torch.from_numpy(grads[i]).cuda() for i in idx]
    outs = [comp.wire_like(x) for x in xs]
    keys = [KEYS[i] for i in idx]
    plans = CastPlanCache(4)
    for step in (4, 5):
        comp.compress_many_sr_into(outs, xs, keys, step, plans=plans)
        for o, i, k in zip(outs, idx, keys):
            assert np.array_equal(_bits(o), sr.sr_round(grads[i], k, step, name))
    assert (plans.built, len(plans)) == (1, 1)                       # hit on the keys
    comp.compress_many_sr_into(outs, xs, [k ^ 1 for k in keys], 6, plans=plans)
    assert (plans.built, len(plans)) == (2, 2)                       # another key misses
    comp.compress_many_into(outs, xs, plans=plans)                   # the plain plan is another
    assert (plans.built, len(plans)) == (3, 3)
    for o, x in zip(outs, xs):
        assert torch.equal(o.cpu(), x.cpu().to(o.dtype))
    # without a cache a plan is built and destroyed inside the call
    comp.compress_many_sr_into(outs, xs, keys, 4)
    for o, i, k in zip(outs, idx, keys):
        assert np.array_equal(_bits(o), sr.sr_round(grads[i], k, 4, name))
    # the decompress over the same tensors and keys finds the SR plan (in
    # place, as push_pull_iteration does) and is the plain decompress
    comp.decompress_many_into(xs, outs, 1, plans=plans, keys=keys)
    assert (plans.built, len(plans)) == (3, 3)
    for x, o in zip(xs, outs):
        assert torch.equal(x, o.float())
    plans.close()
