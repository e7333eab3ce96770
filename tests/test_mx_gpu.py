"""Block-scaled 8- and 4-bit wires on the GPU:
byteps_reduce_mx_* (prophet_amd/csrc/bpsr_k_mx.hip) against prophet_amd/mx.py,
byte for byte — there is no tolerance in the scheme.

Every operand lies between 0xA5 bytes and the whole buffers are compared.
Sizes go around a b128 vector, a block of 32, a wave's run and the
4,096-element tile, as plans of one segment and of every size together, with
the float32 operands 16-byte aligned (vector paths) and 4 bytes off (element
paths), two compress steps a plan so that a residual the device wrote feeds the
next.  The inputs: `edge` tiles the CPU file's blocks (every code, midpoint,
saturation, X == 0, non-finite); `scaled` is normals times 2^-40..2^40 a block;
`extreme` alternates blocks of f32 subnormals with blocks near FLT_MAX."""
import numpy as np
import pytest

from prophet_amd import mx, reducer
from prophet_amd.compression import CastPlanCache
from test_mx import COMP, FMTS, edge_values

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TILE = 4096
SIZES = [1, 3, 4, 5, 31, 32, 33, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 37]
PAD, SENT = 256, 0xA5
F = np.float32


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


def make_inputs(kind, rng, n, fmt):
    """(g, r) of n elements."""
    blocks = -(-n // 32)
    if kind == "edge":
        return np.resize(edge_values(fmt), n), np.zeros(n, F)
    if kind == "scaled":
        scale = np.repeat(np.exp2(rng.integers(-40, 41, blocks)), 32)[:n].astype(F)
        return rng.standard_normal(n).astype(F) * scale, rng.standard_normal(n).astype(F) * scale
    scale = np.repeat(np.where(np.arange(blocks) % 2, F(2.0 ** 126), F(2.0 ** -140)), 32)[:n]
    return (rng.uniform(-1.9, 1.9, n) * scale).astype(F), np.zeros(n, F)


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("kind", ["edge", "scaled", "extreme"])
@pytest.mark.parametrize("n", SIZES + [0], ids=lambda n: str(n) if n else "all")
@pytest.mark.parametrize("fmt", FMTS)
def test_compress_two_steps(red, fmt, n, kind, off):
    """n == 0: every size as the segments of ONE plan, an empty one among them."""
    rng = np.random.default_rng(n * 8 + off)
    shape = [n] if n else SIZES + [0]
    host = [make_inputs(kind, rng, m, fmt) for m in shape]
    G = [Buf(g, off) for g, _ in host]
    R = [Buf(r, off) for _, r in host]
    P = [Buf(np.full(mx.payload_bytes(m, fmt), 0x5A, np.uint8)) for m in shape]
    plan = red.mx_plan([(g.view(torch.float32), r.view(torch.float32), p.view(), m)
                        for g, r, p, m in zip(G, R, P, shape)], fmt)
    res = [r for _, r in host]
    for step in range(2):
        plan.compress()
        torch.cuda.synchronize()
        for i, m in enumerate(shape):
            pay, res[i] = mx.compress(host[i][0], res[i], fmt)
            P[i].expect(pay)
            R[i].expect(res[i])
            for b, name in ((P[i], "payload"), (R[i], "residual"), (G[i], "gradient")):
                b.check(f"step {step}, n {m}, {name}")
    plan.close()


def fold_sources(rng, n, nsrc, fmt):
    """`nsrc` payloads with garbage headers.  Elements 7, 4095 and 4096 hold
    2^24, 1 and -2^24 in turn, so the order shows; source 1 carries an X == 255
    block where n allows."""
    out = []
    for s in range(nsrc):
        g = make_inputs("scaled", rng, n, fmt)[0]
        g[[i for i in (7, TILE - 1, TILE) if i < n]] = [2.0 ** 24, 1.0, -2.0 ** 24][s % 3]
        if s == 1 and n > 40:
            g[40] = np.inf
        pay = mx.compress(g, np.zeros(n, F), fmt)[0]
        pay[:16] = np.array([0xdeadbeef, 0xffffffff, 0x12345678, 0xa5a5a5a5], "<u4").view(np.uint8)
        out.append(pay)
    return out


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("fmt", FMTS)
def test_fold(red, fmt, nsrc, divisor, off):
    rng = np.random.default_rng(nsrc * 16 + divisor + off)
    shape = SIZES + [0]
    srcs = [fold_sources(rng, n, nsrc, fmt) for n in shape]
    S = [[Buf(p) for p in ps] for ps in srcs]
    O = [Buf(np.full(n, 7.0, F), off) for n in shape]
    plan = red.mx_fold_plan([(o.view(torch.float32), [p.view() for p in ps], n)
                             for o, ps, n in zip(O, S, shape)], nsrc, fmt)
    plan.launch(divisor)
    torch.cuda.synchronize()
    plan.close()
    for o, ps, hs, n in zip(O, S, srcs, shape):
        o.expect(mx.fold(hs, n, fmt, divisor))
        o.check(f"n {n}, output")
        for s, p in enumerate(ps):
            p.check(f"n {n}, source {s}")


@pytest.mark.parametrize("fmt", FMTS)
def test_compressor_device_path(fmt):
    C = COMP[fmt]
    rng = np.random.default_rng(5)
    gs = [rng.standard_normal(n).astype(F) for n in (1000, TILE + 5)]
    T = [torch.from_numpy(g).cuda() for g in gs]
    P = [C.payload_like(t) for t in T]
    R = [C.residual_like(t) for t in T]
    plans, refs = CastPlanCache(4), [np.zeros(g.size, F) for g in gs]
    for _ in range(2):
        C.compress_many_ef_into(P, R, T, plans=plans)
        for i, g in enumerate(gs):
            pay, refs[i] = mx.compress(g, refs[i], fmt)
            assert np.array_equal(P[i].cpu().numpy(), pay)
            assert np.array_equal(R[i].cpu().numpy(), refs[i])
    assert plans.built == 1
    outs = [torch.empty_like(t) for t in T]
    C.fold_many_into(outs, [[p, p.clone()] for p in P], 2, plans=plans)
    for o, p, g in zip(outs, P, gs):
        h = p.cpu().numpy()
        assert np.array_equal(o.cpu().numpy(), mx.fold([h, h], g.size, fmt, 2))
    plans.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_refused_calls_leave_every_buffer(red, fmt):
    n = TILE + 1
    g, r, o = Buf(np.ones(n, F)), Buf(np.ones(n, F)), Buf(np.ones(n, F))
    p, q = (Buf(np.full(mx.payload_bytes(n, fmt), 0x5A, np.uint8)) for _ in range(2))
    f32 = torch.float32
    comp = red.mx_plan([(g.view(f32), r.view(f32), p.view(), n)], fmt)
    fold = red.mx_fold_plan([(o.view(f32), [q.view()], n)], 1, fmt)
    lib = red.lib
    assert lib.byteps_reduce_mx_fold_plan_launch(comp.handle, 1, None) == reducer.EARGS
    assert lib.byteps_reduce_mx_plan_compress(fold.handle, None) == reducer.EARGS
    assert lib.byteps_reduce_mx_fold_plan_launch(fold.handle, 0, None) == reducer.EARGS
    for segs in ([(g.view(f32), g.view(f32), p.view(), n)],             # grad is the residual
                 [(g.view(f32), r.view(f32), p.view()[16:], n)]):        # a payload too short
        with pytest.raises((reducer.ReduceError, ValueError)):
            red.mx_plan(segs, fmt)
    with pytest.raises(reducer.ReduceError):
        red.mx_fold_plan([(o.view(f32), [q.view()] * 17, n)], 17, fmt)
    torch.cuda.synchronize()
    comp.close()
    fold.close()
    for b, name in ((g, "g"), (r, "r"), (o, "out"), (p, "payload"), (q, "source")):
        b.check(name)
