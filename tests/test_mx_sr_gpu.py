"""The stateless block-scaled wires on the GPU:
byteps_reduce_mx_sr_* and byteps_reduce_mx_rht_fold_*
(prophet_amd/csrc/bpsr_k_mx_sr.hip) against prophet_amd/mx_sr.py, byte for byte
— there is no tolerance in the scheme.

Every operand lies between 0xA5 bytes and the whole buffers are compared.
Sizes go around a b128 vector, a block of 32, a wave's run and the
4,096-element tile, as plans of one segment and of every size together, the
gradients 16-byte aligned and 4 bytes off, two steps a plan, a key a segment.
The inputs: `edge` tiles the CPU file's blocks; `scaled` is normals times
2^-40..2^40 a block; `extreme` alternates blocks of f32 subnormals with blocks
near FLT_MAX / 32 (a rotated block's butterflies add up to 32 of them)."""
import numpy as np
import pytest

from prophet_amd import mx, mx_sr, reducer
from prophet_amd.compression import CastPlanCache
from test_mx_gpu import Buf
from test_mx_sr import COMP, case, edge_blocks

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TILE = 4096
SIZES = [0, 1, 3, 4, 5, 31, 32, 33, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 33]
F = np.float32


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return reducer.GpuReducer(device=0)


def make_input(kind, rng, n, fmt):
    blocks = -(-n // 32)
    if kind == "edge":
        return np.resize(edge_blocks(fmt), n)
    if kind == "scaled":
        scale = np.repeat(np.exp2(rng.integers(-40, 41, blocks)), 32)[:n].astype(F)
        return rng.standard_normal(n).astype(F) * scale
    scale = np.repeat(np.where(np.arange(blocks) % 2, F(2.0 ** 122), F(2.0 ** -140)), 32)[:n]
    return (rng.uniform(-1.9, 1.9, n) * scale).astype(F)


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("kind", ["edge", "scaled", "extreme"])
@pytest.mark.parametrize("n", SIZES[1:] + [None], ids=lambda n: str(n) if n else "all")
@case
def test_compress_two_steps(red, fmt, rot, n, kind, off):
    """n None: every size as the segments of ONE plan, the empty one among them."""
    rng = np.random.default_rng((n or 0) * 8 + off)
    shape = [n] if n else SIZES
    host = [make_input(kind, rng, m, fmt) for m in shape]
    keys = [(0x9e3779b9 * (i + 1) & 0xffffffff, 0xdeadbeef + i) for i in range(len(shape))]
    G = [Buf(g, off) for g in host]
    P = [Buf(np.full(mx.payload_bytes(m, fmt), 0x5A, np.uint8)) for m in shape]
    plan = red.mx_sr_plan([(g.view(torch.float32), p.view(), m, k, rk)
                           for g, p, m, (k, rk) in zip(G, P, shape, keys)], fmt, rot)
    for step in (0, 0xfffffffe):
        plan.compress(step)
        torch.cuda.synchronize()
        for i, m in enumerate(shape):
            P[i].expect(mx_sr.compress(host[i], fmt, keys[i][0], step, rot, keys[i][1]))
            P[i].check(f"step {step}, n {m}, payload")
            G[i].check(f"step {step}, n {m}, gradient")
    plan.close()


def fold_sources(rng, n, nsrc, fmt, rot, rot_key, step):
    """`nsrc` payloads of one rotation with garbage headers; source 1 carries an
    X == 255 block where n allows."""
    out = []
    for s in range(nsrc):
        g = make_input("scaled", rng, n, fmt)
        if s == 1 and n > 40:
            g[40] = np.inf
        pay = mx_sr.compress(g, fmt, 100 + s, step, rot, rot_key)
        pay[:16] = np.array([0xdeadbeef, 0xffffffff, 0x12345678, 0xa5a5a5a5], "<u4").view(np.uint8)
        out.append(pay)
    return out


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("nsrc", [1, 2, 8, 9, 16])
@case
def test_fold(red, fmt, rot, nsrc, divisor, off):
    """Rotated payloads through the rotated fold; unrotated ones through the
    block-scaled fold plan there was."""
    rng = np.random.default_rng(nsrc * 16 + divisor + off)
    step, rks = 7, [0x1000 + i for i in range(len(SIZES))]
    srcs = [fold_sources(rng, n, nsrc, fmt, rot, rk, step) for n, rk in zip(SIZES, rks)]
    S = [[Buf(p) for p in ps] for ps in srcs]
    O = [Buf(np.full(n, 7.0, F), off) for n in SIZES]
    if rot:
        plan = red.mx_rht_fold_plan([(o.view(torch.float32), [p.view() for p in ps], n, rk)
                                     for o, ps, n, rk in zip(O, S, SIZES, rks)], nsrc, fmt)
        plan.launch(divisor, step)
    else:
        plan = red.mx_fold_plan([(o.view(torch.float32), [p.view() for p in ps], n)
                                 for o, ps, n in zip(O, S, SIZES)], nsrc, fmt)
        plan.launch(divisor)
    torch.cuda.synchronize()
    plan.close()
    for o, ps, hs, n, rk in zip(O, S, srcs, SIZES, rks):
        o.expect(mx_sr.fold(hs, n, fmt, divisor, rot, rk, step))
        o.check(f"n {n}, output")
        for s, p in enumerate(ps):
            p.check(f"n {n}, source {s}")


@case
def test_compressor_device_path(fmt, rot):
    C = COMP[(fmt, rot)]
    rng = np.random.default_rng(5)
    gs = [rng.standard_normal(n).astype(F) for n in (1000, TILE + 5)]
    T = [torch.from_numpy(g).cuda() for g in gs]
    P, Q = ([C.payload_like(t) for t in T] for _ in range(2))
    plans, rks = CastPlanCache(4), [11, 12]
    for step in (0, 1):
        C.compress_many_sr_into(P, T, [1, 2], step, rks, plans=plans)
    C.compress_many_sr_into(Q, T, [3, 4], 1, rks, plans=plans)
    assert plans.built == 2
    host = [[mx_sr.compress(g, fmt, k, 1, rot, rk) for k in ks]
            for g, ks, rk in zip(gs, ((1, 3), (2, 4)), rks)]
    for p, q, h in zip(P, Q, host):
        assert np.array_equal(p.cpu().numpy(), h[0]) and np.array_equal(q.cpu().numpy(), h[1])
    outs = [torch.empty_like(t) for t in T]
    C.fold_many_into(outs, [[p, q] for p, q in zip(P, Q)], 2, rot_keys=rks, step=1, plans=plans)
    for o, h, g, rk in zip(outs, host, gs, rks):
        assert np.array_equal(o.cpu().numpy(), mx_sr.fold(h, g.size, fmt, 2, rot, rk, 1))
    plans.close()


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_refused_calls_leave_every_buffer(red, fmt):
    n = TILE + 1
    g, r, o = Buf(np.ones(n, F)), Buf(np.ones(n, F)), Buf(np.ones(n, F))
    p, q = (Buf(np.full(mx.payload_bytes(n, fmt), 0x5A, np.uint8)) for _ in range(2))
    f32 = torch.float32
    plans = {"sr": red.mx_sr_plan([(g.view(f32), p.view(), n, 1, 2)], fmt, True),
             "rht": red.mx_rht_fold_plan([(o.view(f32), [q.view()], n, 2)], 1, fmt),
             "ef": red.mx_plan([(g.view(f32), r.view(f32), p.view(), n)], fmt),
             "fold": red.mx_fold_plan([(o.view(f32), [q.view()], n)], 1, fmt)}
    lib = red.lib
    for name, plan in plans.items():                 # every launch on a plan of another kind
        h = plan.handle
        assert name == "sr" or lib.byteps_reduce_mx_sr_plan_compress(h, 0, None) == reducer.EARGS
        assert name == "rht" or \
            lib.byteps_reduce_mx_rht_fold_plan_launch(h, 1, 0, None) == reducer.EARGS
        assert name == "ef" or lib.byteps_reduce_mx_plan_compress(h, None) == reducer.EARGS
        assert name == "fold" or lib.byteps_reduce_mx_fold_plan_launch(h, 1, None) == reducer.EARGS
    assert lib.byteps_reduce_mx_rht_fold_plan_launch(plans["rht"].handle, 0, 0, None) == reducer.EARGS
    with pytest.raises((reducer.ReduceError, ValueError)):
        red.mx_sr_plan([(g.view(f32), p.view()[16:], n, 1, 2)], fmt)     # a payload too short
    with pytest.raises(reducer.ReduceError):
        red.mx_rht_fold_plan([(o.view(f32), [q.view()] * 17, n, 2)], 17, fmt)
    torch.cuda.synchronize()
    for plan in plans.values():
        plan.close()
    for b, name in ((g, "g"), (r, "r"), (o, "out"), (p, "payload"), (q, "source")):
        b.check(name)
