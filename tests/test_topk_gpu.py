"""Top-k sparsification with error feedback on the GPU:
byteps_reduce_topk_* (prophet_amd/csrc/bpsr_k_topk.hip) against
prophet_amd/topk.py, byte for byte — there is no tolerance in the scheme.

Every operand lies between 0xA5 bytes and the whole buffers are compared.
Sizes go around a b128 vector, a wave's run and the 4,096-element tile, as
plans of one segment and of every (n, k) together, with the float32 operands
16-byte aligned (vector paths) and 4 bytes off (element paths), two compress
steps a plan.  The inputs: `ties` draws magnitudes from eight values, so the
threshold's ties straddle tiles and need_eq cuts inside one; `digit0/1/2` are
keys that differ in one radix digit only, so each pass decides alone;
`general` is normals with a NaN, an inf and both zeros planted."""
import numpy as np
import pytest

from prophet_amd import reducer, topk
from prophet_amd.compression import CastPlanCache, Compression

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TILE = 4096
SIZES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 37]
PAD, SENT = 256, 0xA5
F = np.float32


def ks(n):
    return sorted({min(n, max(1, k)) for k in (1, 2, -(-n // 100), n // 2, n - 1, n)})


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return reducer.GpuReducer(device=0)


class Buf:
    """`data` (any numpy array) on the device at 16-byte alignment + `off`,
    between PAD sentinel bytes; `want` is the host image to compare with."""

    def __init__(self, data, off=0):
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        self.lo, self.hi = PAD + off, PAD + off + raw.size
        self.want = np.full(self.hi + PAD, SENT, dtype=np.uint8)
        self.want[self.lo:self.hi] = raw
        self.dev = torch.from_numpy(self.want.copy()).cuda()

    def view(self, dtype=torch.uint8):
        return self.dev[self.lo:self.hi].view(dtype)

    def expect(self, data):
        self.want[self.lo:self.hi] = np.ascontiguousarray(data).reshape(-1).view(np.uint8)

    def check(self, what):
        got = self.dev.cpu().numpy()
        bad = np.flatnonzero(got != self.want)
        assert bad.size == 0, f"{what}: first differing byte {bad[0] - self.lo} of the operand"


def make_inputs(kind, rng, n):
    zero = np.zeros(n, F)
    if kind == "ties":
        mags = np.array([0.0, 0.25, 0.5, 1, 1.5, 2, 3, 1e-40], F)      # a subnormal among them
        return mags[rng.integers(0, 8, n)] * rng.choice(np.array([-1, 1], F), n), zero
    if kind.startswith("digit"):
        shift = {"digit0": 20, "digit1": 10, "digit2": 0}[kind]
        lo, hi = (1, 0x7f8) if shift == 20 else (0, 1024)               # finite exponents
        bits = (0 if shift == 20 else 0x3f800000) | (rng.integers(lo, hi, n) << shift)
        bits |= rng.integers(0, 2, n) << 31
        return bits.astype(np.uint32).view(F), zero
    g = rng.standard_normal(n).astype(F)
    r = rng.standard_normal(n).astype(F) * F(0.1)
    if n > 8:
        g[1], g[3] = np.nan, -np.inf
        g[5], r[5], g[6], r[6] = 0.0, 0.0, -0.0, -0.0
    return g, r


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("kind", ["ties", "digit0", "digit1", "digit2", "general"])
@pytest.mark.parametrize("n", SIZES + [0], ids=lambda n: str(n) if n else "all")
def test_compress_two_steps(red, n, kind, off):
    """n == 0: every (n, k) of SIZES as the segments of ONE plan, an empty
    segment among them; else one plan per k."""
    rng = np.random.default_rng(n * 8 + off)
    plans = [[(n, k)] for k in ks(n)] if n else [[(m, k) for m in SIZES for k in ks(m)] + [(0, 0)]]
    for shape in plans:
        host = [make_inputs(kind, rng, m) for m, _ in shape]
        G = [Buf(g, off) for g, _ in host]
        R = [Buf(r, off) for _, r in host]
        P = [Buf(np.full(topk.payload_bytes(k), 0x5A, np.uint8)) for _, k in shape]
        plan = red.topk_plan([(g.view(torch.float32), r.view(torch.float32), p.view(), m, k)
                              for g, r, p, (m, k) in zip(G, R, P, shape)])
        res = [r for _, r in host]
        for step in range(2):
            plan.compress()
            torch.cuda.synchronize()
            for i, (m, k) in enumerate(shape):
                pay, res[i] = topk.compress(host[i][0], res[i], k)
                P[i].expect(pay)
                R[i].expect(res[i])
                for b, name in ((P[i], "payload"), (R[i], "residual"), (G[i], "gradient")):
                    b.check(f"step {step}, n {m}, k {k}, {name}")
        plan.close()


def fold_sources(rng, n, k, nsrc):
    """`nsrc` payloads of k entries with garbage headers.  Where n allows:
    source 0 lies in tile 1 alone and source 1 has nothing there; the others
    hold 7, 4095 and 4096, where 2^24, 1 and -2^24 meet, so the order shows."""
    out = []
    for s in range(nsrc):
        forced = np.array([i for i in (7, TILE - 1, TILE) if i < n and s >= 2][:k], np.int64)
        pool = np.arange(n)
        if n > 2 * TILE and s == 0:
            pool = pool[TILE:2 * TILE]
        elif n > 2 * TILE and s == 1:
            pool = np.concatenate([pool[:TILE], pool[2 * TILE:]])
        rest = rng.choice(np.setdiff1d(pool, forced), k - forced.size, replace=False)
        idx = np.sort(np.concatenate([forced, rest]))
        val = rng.integers(-8, 9, k).astype(F)
        val[np.isin(idx, forced)] = [2.0 ** 24, 1.0, -2.0 ** 24][s % 3]
        head = np.array([0xdeadbeef, 0xffffffff, 0x12345678, 0xa5a5a5a5], "<u4")
        out.append(np.concatenate([head, idx.astype("<u4"), val.view("<u4")]).view(np.uint8))
    return out


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 8, 16])
def test_fold(red, nsrc, divisor, off):
    rng = np.random.default_rng(nsrc * 16 + divisor + off)
    shape = [(1, 1), (63, 63), (TILE + 1, 41), (3 * TILE + 37, 300), (0, 0)]
    srcs = [fold_sources(rng, n, k, nsrc) for n, k in shape]
    S = [[Buf(p) for p in ps] for ps in srcs]
    O = [Buf(np.full(n, 7.0, F), off) for n, _ in shape]
    plan = red.topk_fold_plan([(o.view(torch.float32), [p.view() for p in ps], n, k)
                               for o, ps, (n, k) in zip(O, S, shape)], nsrc)
    plan.launch(divisor)
    torch.cuda.synchronize()
    plan.close()
    for o, ps, hs, (n, k) in zip(O, S, srcs, shape):
        o.expect(topk.fold(hs, n, divisor, k))
        o.check(f"n {n}, k {k}, output")
        for s, p in enumerate(ps):
            p.check(f"n {n}, source {s}")


def test_compressor_device_path():
    TK = Compression.topk_ef
    rng = np.random.default_rng(5)
    gs = [rng.standard_normal(n).astype(F) for n in (1000, TILE + 5)]
    T = [torch.from_numpy(g).cuda() for g in gs]
    P = [TK.payload_like(t, 0.01) for t in T]
    R = [TK.residual_like(t) for t in T]
    assert [topk.k_of(p) for p in P] == [10, 42]
    plans, refs = CastPlanCache(4), [np.zeros(g.size, F) for g in gs]
    for _ in range(2):
        TK.compress_many_ef_into(P, R, T, plans=plans)
        for i, g in enumerate(gs):
            pay, refs[i] = topk.compress(g, refs[i], topk.k_of(P[i]))
            assert np.array_equal(P[i].cpu().numpy(), pay)
            assert np.array_equal(R[i].cpu().numpy(), refs[i])
    assert plans.built == 1
    outs = [torch.empty_like(t) for t in T]
    TK.fold_many_into(outs, [[p, p.clone()] for p in P], 2, plans=plans)
    for o, p, g in zip(outs, P, gs):
        h = p.cpu().numpy()
        assert np.array_equal(o.cpu().numpy(), topk.fold([h, h], g.size, 2))
    plans.close()


def test_refused_calls_leave_every_buffer(red):
    n, k = TILE + 1, 9
    g, r, o = Buf(np.ones(n, F)), Buf(np.ones(n, F)), Buf(np.ones(n, F))
    p, q = Buf(np.full(topk.payload_bytes(k), 0x5A, np.uint8)), Buf(np.zeros(16 + 8 * k, np.uint8))
    f32 = torch.float32
    comp = red.topk_plan([(g.view(f32), r.view(f32), p.view(), n, k)])
    fold = red.topk_fold_plan([(o.view(f32), [q.view()], n, k)], 1)
    lib = red.lib
    assert lib.byteps_reduce_topk_fold_plan_launch(comp.handle, 1, None) == reducer.EARGS
    assert lib.byteps_reduce_topk_plan_compress(fold.handle, None) == reducer.EARGS
    assert lib.byteps_reduce_topk_fold_plan_launch(fold.handle, 0, None) == reducer.EARGS
    for segs in ([(g.view(f32), g.view(f32), p.view(), n, k)],           # grad is the residual
                 [(g.view(f32), r.view(f32), p.view(), n, n + 1)],
                 [(g.view(f32), r.view(f32), p.view()[8:], n, k - 1)]):   # payload alignment
        with pytest.raises((reducer.ReduceError, ValueError)):
            red.topk_plan(segs)
    with pytest.raises(reducer.ReduceError):
        red.topk_fold_plan([(o.view(f32), [q.view(), q.view()], n, k)], 2)
    with pytest.raises(reducer.ReduceError):
        red.topk_fold_plan([(o.view(f32), [q.view()] * 17, n, k)], 17)
    torch.cuda.synchronize()
    comp.close()
    fold.close()
    for b, name in ((g, "g"), (r, "r"), (o, "out"), (p, "payload"), (q, "source")):
        b.check(name)
