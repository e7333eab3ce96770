"""Error-feedback cast plans (byteps_reduce_cast_plan_create_ef; the plan kernel
of prophet_amd/csrc/bpsr_cast_plan.h under the scheme of bpsr_cast_ef.h) on the
GPU: one launch over an empty, a
1-element, a never-co-aligned, a partial-tile and one- and several-tile
segments against one ``compress_ef`` per segment (wire and residual, bit for
bit, sentinel bytes between the segments intact) and against the host
definition; the EF plan's decompress against the plain plan's with divisors 1
and 3, residuals untouched; the argument errors, all before any launch; and a
``CastPlanCache`` asked for a plain and an EF plan over the same tensors."""
import numpy as np
import pytest

from prophet_amd import reducer
from prophet_amd.compression import CastPlanCache, Compression
from prophet_amd.dtypes import DType
from prophet_amd.reducer import GpuReducer

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

F32 = DType.FLOAT32
WIRES = [(DType.FLOAT16, torch.float16), (DType.BFLOAT16, torch.bfloat16)]
IDS = ["fp16", "bf16"]
TILE = 256 * 8
SENTINEL = 0xA5
GAP = 64            # sentinel bytes between operands, at least

# (elements, wide offset, wire offset, residual offset), offsets in BYTES past
# a 256-byte boundary
LAYOUT = [
    (0, 0, 0, 0),                    # empty
    (1, 0, 0, 0),                    # one element
    (TILE + 100, 0, 0, 4),           # the residual never co-aligns: element path
    (777, 0, 0, 0),                  # a partial tile and a tail
    (TILE, 0, 0, 0),                 # exactly one full tile
    (3 * TILE + 13, 4, 2, 4),        # several full tiles after a 7-element head
    (5 * TILE + 8 * 31 + 5, 12, 6, 12),   # full tiles, a partial one, head and tail
    (300, 0, 0, 2),                  # residual element-misaligned: byte-wise element path
]


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return GpuReducer(device=0)


def host_ef(g, r, wire):
    c = g + r
    w = c.to(wire)
    b = w.to(torch.float32)
    return w, torch.where(torch.isfinite(b), c - b, torch.zeros_like(c))


def _arena(nbytes):
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    skip = (-raw.data_ptr()) % 256
    a = raw[skip:skip + nbytes]
    a.fill_(SENTINEL)
    return a


def _place(arena, cursor, nbytes, off):
    """[begin, end) of an operand `off` bytes past the next 256-byte boundary
    that leaves GAP sentinel bytes before it."""
    begin = (cursor + GAP + 255) // 256 * 256 + off
    return begin, begin + nbytes


class Arena:
    """The operands of LAYOUT as byte ranges of one sentinel-filled buffer."""

    def __init__(self, g, r):
        total = sum(256 + GAP + n * 10 + 768 for n, *_ in LAYOUT) + 1024
        self.buf = _arena(total)
        self.segs = []                            # (n, wide, wire, resid) byte ranges
        cur, e0 = 0, 0
        for n, wo, ho, ro in LAYOUT:
            w = _place(self.buf, cur, n * 4, wo)
            h = _place(self.buf, w[1], n * 2, ho)
            q = _place(self.buf, h[1], n * 4, ro)
            cur = q[1]
            self.segs.append((n, w, h, q, e0))
            e0 += n
        self.g, self.r = g, r
        self.used = torch.zeros(total, dtype=torch.bool)
        for n, w, h, q, _ in self.segs:
            for a, b in (w, h, q):
                self.used[a:b] = True
        self.reset()

    def reset(self):
        self.buf.fill_(SENTINEL)
        for n, w, h, q, e0 in self.segs:
            self.buf[w[0]:w[1]].copy_(self.g[e0:e0 + n].contiguous().view(torch.uint8))
            self.buf[q[0]:q[1]].copy_(self.r[e0:e0 + n].contiguous().view(torch.uint8))

    def ptr(self, rng):
        return self.buf.data_ptr() + rng[0]

    def quads(self):
        return [(self.ptr(w), self.ptr(h), n, self.ptr(q)) for n, w, h, q, _ in self.segs]

    def bytes_of(self, rng):
        return self.buf[rng[0]:rng[1]].cpu()

    def sentinels_intact(self):
        return bool((self.buf.cpu()[~self.used] == SENTINEL).all())


@pytest.fixture(scope="module")
def values():
    rng = np.random.default_rng(41)
    n = sum(x[0] for x in LAYOUT)
    with np.errstate(over="ignore"):
        g = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 18, n))).astype(np.float32)
    g[:1] = 65520.0
    g[5:9] = [np.inf, -np.inf, 1e-8, -0.0]
    r = (g * np.float32(2.0 ** -10) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    r[~np.isfinite(r)] = 0
    return torch.from_numpy(g).cuda(), torch.from_numpy(r).cuda()


@pytest.mark.parametrize("wd,wt", WIRES, ids=IDS)
def test_plan_compress_is_one_compress_ef_per_segment(red, values, wd, wt):
    g, r = values
    ar = Arena(g, r)
    s = torch.cuda.current_stream()
    # one compress_ef per segment
    for n, w, h, q, _ in ar.segs:
        red.compress_ef(ar.ptr(h), ar.ptr(q), ar.ptr(w), n, F32, wd, stream=s)
    torch.cuda.synchronize()
    single = [(ar.bytes_of(h), ar.bytes_of(q)) for n, w, h, q, _ in ar.segs]
    assert ar.sentinels_intact()
    # and against the host definition
    gc, rc = g.cpu(), r.cpu()
    for (n, w, h, q, e0), (hb, qb) in zip(ar.segs, single):
        ww, wr = host_ef(gc[e0:e0 + n], rc[e0:e0 + n], wt)
        assert torch.equal(hb, ww.view(torch.uint8)) and torch.equal(qb, wr.view(torch.uint8)), n
    # the plan: the same bytes from one launch
    ar.reset()
    plan = red.cast_plan(ar.quads(), F32, wd)
    assert plan.error_feedback
    plan.compress(stream=s)
    torch.cuda.synchronize()
    for (n, w, h, q, e0), (hb, qb) in zip(ar.segs, single):
        assert torch.equal(ar.bytes_of(h), hb), n
        assert torch.equal(ar.bytes_of(q), qb), n
        assert torch.equal(ar.bytes_of(w), g[e0:e0 + n].cpu().view(torch.uint8))   # src untouched
    assert ar.sentinels_intact()
    # a second launch carries the residual on: again one compress_ef per segment
    plan.compress(stream=s)
    torch.cuda.synchronize()
    twice = [(ar.bytes_of(h), ar.bytes_of(q)) for n, w, h, q, _ in ar.segs]
    ar.reset()
    for _k in range(2):
        for n, w, h, q, _ in ar.segs:
            red.compress_ef(ar.ptr(h), ar.ptr(q), ar.ptr(w), n, F32, wd, stream=s)
    torch.cuda.synchronize()
    for (n, w, h, q, _), (hb, qb) in zip(ar.segs, twice):
        assert torch.equal(ar.bytes_of(h), hb) and torch.equal(ar.bytes_of(q), qb), n
    plan.close()


@pytest.mark.parametrize("wd,wt", WIRES, ids=IDS)
def test_plan_decompress_is_the_plain_one_and_leaves_the_residuals(red, values, wd, wt):
    g, r = values
    ar = Arena(g, r)
    s = torch.cuda.current_stream()
    ef = red.cast_plan(ar.quads(), F32, wd)
    plain = red.cast_plan([(w, h, n) for w, h, n, _ in ar.quads()], F32, wd)
    assert not plain.error_feedback
    ef.compress(stream=s)
    torch.cuda.synchronize()
    resid = [ar.bytes_of(q) for n, w, h, q, _ in ar.segs]
    for d in (1, 3):
        plain.decompress(d, stream=s)
        torch.cuda.synchronize()
        want = [ar.bytes_of(w) for n, w, h, q, _ in ar.segs]
        for n, w, h, q, _ in ar.segs:
            ar.buf[w[0]:w[1]].fill_(0x5A)
        ef.decompress(d, stream=s)
        torch.cuda.synchronize()
        for (n, w, h, q, _), wb, qb in zip(ar.segs, want, resid):
            assert torch.equal(ar.bytes_of(w), wb), (d, n)
            assert torch.equal(ar.bytes_of(q), qb), (d, n)            # residuals untouched
        assert ar.sentinels_intact()
    ef.close()
    plain.close()


def test_argument_errors_raise_before_any_launch(red):
    n = 1000
    wide, res = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    wide2, res2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    wire = torch.zeros(n, dtype=torch.float16, device="cuda")
    wire2 = torch.zeros(n, dtype=torch.float16, device="cuda")
    ok = [(wide, wire, n, res), (wide2, wire2, n, res2)]

    def code(segs, dt=F32, wd=DType.FLOAT16):
        with pytest.raises(reducer.ReduceError) as e:
            red.cast_plan(segs, dt, wd)
        return e.value.code

    # overlap between any two of the 3 * nsegs ranges
    assert code([(wide, wire, n, wide)]) == reducer.EARGS
    assert code([ok[0], (wide2, wire2, n, res)]) == reducer.EARGS
    assert code([ok[0], (res, wire2, n, res2)]) == reducer.EARGS
    assert code([ok[0], (wide2, wire2, n - 4, res[4:])]) == reducer.EARGS
    assert code([ok[0], (wide2, wire, n, res2)]) == reducer.EARGS
    assert code([ok[0], (wide2, wire2.data_ptr(), n, wire2.data_ptr() + 2 * n - 2)]) == reducer.EARGS
    # a null residual, a non-f32 wide dtype, a wire that is none
    assert code([ok[0], (wide2, wire2, n, None)]) == reducer.EARGS
    wide64 = torch.zeros(n, dtype=torch.float64, device="cuda")
    assert code([(wide64, wire, n, res)], DType.FLOAT64) == reducer.EDTYPE
    assert code([(wire2, wire, n, res)], DType.BFLOAT16) == reducer.EDTYPE
    assert code(ok, F32, F32) == reducer.EDTYPE
    with pytest.raises(ValueError):
        red.cast_plan([(wide, wire, n, res[:-1])], F32)                # residual one element short
    with pytest.raises(ValueError):
        red.cast_plan([ok[0], (wide2, wire2, n)], F32)                 # residuals: all or none
    # empty plans launch nothing
    for segs in ([], [(None, None, 0, None)]):
        p = red.cast_plan(segs, F32, DType.BFLOAT16)
        p.compress()
        p.decompress(3)
        p.close()
    torch.cuda.synchronize()
    for t in (wide, res, wide2, res2, wire.float(), wire2.float()):
        assert float(t.abs().sum()) == 0.0


def test_compress_many_and_the_plan_cache(red, values):
    g, r = values
    sizes = [1, 777, TILE, 3 * TILE + 13]
    for comp, wt in ((Compression.fp16_ef, torch.float16), (Compression.bf16_ef, torch.bfloat16)):
        xs, e0 = [], 0
        for n in sizes:
            xs.append(g[e0:e0 + n].clone())
            e0 += n
        ress = [r[:n].clone() for n in sizes]
        outs = [comp.wire_like(x) for x in xs]
        plans = CastPlanCache(4)
        comp.compress_many_ef_into(outs, ress, xs, plans=plans)
        assert (plans.built, len(plans)) == (1, 1)
        for x, o, q in zip(xs, outs, ress):
            ww, wr = host_ef(x.cpu(), r[:x.numel()].cpu(), wt)
            assert torch.equal(o.cpu().view(torch.int16), ww.view(torch.int16))
            assert torch.equal(q.cpu().view(torch.int32), wr.view(torch.int32))
        # the same plan decompresses (named by its residuals) and is found again
        # (in place, as push_pull_iteration does: the wide side is the plan's own)
        comp.decompress_many_into(xs, outs, 3, plans=plans, residuals=ress)
        comp.compress_many_ef_into(outs, ress, xs, plans=plans)
        assert (plans.built, len(plans)) == (1, 1)
        # without residuals it is the plain plan: another one
        comp.decompress_many_into(xs, outs, 3, plans=plans)
        assert (plans.built, len(plans)) == (2, 2)
        # a moved residual misses
        moved = [q.clone() for q in ress]
        comp.compress_many_ef_into(outs, moved, xs, plans=plans)
        assert (plans.built, len(plans)) == (3, 3)
        # and without a cache a plan is built and destroyed in the call
        ress2 = [r[:n].clone() for n in sizes]
        outs2 = [comp.wire_like(x) for x in xs]
        comp.compress_many_ef_into(outs2, ress2, xs)
        torch.cuda.synchronize()
        for x, o, q in zip(xs, outs2, ress2):
            ww, wr = host_ef(x.cpu(), r[:x.numel()].cpu(), wt)
            assert torch.equal(o.cpu().view(torch.int16), ww.view(torch.int16))
            assert torch.equal(q.cpu().view(torch.int32), wr.view(torch.int32))
        plans.close()
