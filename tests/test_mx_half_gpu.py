"""The block-scaled wires over float16 and bfloat16 tensors on the GPU (DESIGN.md
§11.16; prophet_amd/csrc/bpsr_k_mx_half.hip) against the numpy definition, byte
for byte, through the compressors: many tensors a call, a float32 one among
them.  Every operand lies between sentinel bytes, 0, 2, 4 or 8 bytes off a
16-byte boundary, and the whole buffers are compared.  Sizes go around a unit of
8, a block of 32 and the 4,096-element tile."""
import numpy as np
import pytest

from prophet_amd import mx, mx_sr
from prophet_amd.compression import CastPlanCache
from test_mx_gpu import Buf
from test_mx_half import COMP, KEY, ROT_KEY, STEP, define_fold, dtypes, half_input, wires

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TILE = 4096
SIZES = [1, 31, 32, 33, TILE - 1, TILE, TILE + 1, 2 * TILE + 40]
F = np.float32


def values(rng, n, dt=None, spread=20):
    """Normals times a power of two a block; with `dt`, where n allows, a block
    with an infinity, one with a NaN, and one of fp16 subnormals or of bf16
    magnitudes next to 2^127 (the stateless wires bump that scale)."""
    v = rng.standard_normal(n) * np.repeat(np.exp2(rng.integers(-spread, 15, -(-n // 32))), 32)[:n]
    if dt and n > 192:
        v[40], v[100] = np.inf, np.nan
        v[128:160] = (rng.integers(-1023, 1024, 32) * 2.0 ** -24 if dt == "float16" else
                      rng.uniform(-1.99, 1.99, 32) * 2.0 ** 127)
    return v


@pytest.mark.parametrize("off", [0, 2, 4, 8])
@dtypes
@wires
def test_compress_many(fmt, kind, dt, off):
    """Every size and a float32 tensor in ONE call, two steps: the second step
    of the error-feedback wires starts from a non-zero residual."""
    rng = np.random.default_rng(off)
    comp, tdt, bf16 = COMP[fmt, kind], getattr(torch, dt), dt == "bfloat16"
    host = [half_input(dt, values(rng, n, dt))[0] for n in SIZES] + [values(rng, 100).astype(F)]
    ns = SIZES + [100]
    G = [Buf(g, off) for g in host[:-1]] + [Buf(host[-1], off and 4)]
    P = [Buf(np.full(mx.payload_bytes(n, fmt), 0x5A, np.uint8)) for n in ns]
    res = [(rng.standard_normal(n) * 2.0 ** -10).astype(F) for n in ns]
    R = [Buf(r, off and 4) for r in res]
    tensors = [g.view(tdt) for g in G[:-1]] + [G[-1].view(torch.float32)]
    keys = [KEY + i for i in range(len(ns))]
    cache = CastPlanCache()
    for step in (3, 4):
        if kind == "ef":
            comp.compress_many_ef_into([p.view() for p in P], [r.view(torch.float32) for r in R],
                                       tensors, cache)
        else:
            comp.compress_many_sr_into([p.view() for p in P], tensors, keys, step,
                                       [ROT_KEY] * len(ns), cache)
        torch.cuda.synchronize()
        for i, n in enumerate(ns):
            half = bf16 and i < len(SIZES)
            if kind == "ef":
                pay, res[i] = mx.compress(host[i], res[i], fmt, half)
                R[i].expect(res[i])
                R[i].check(f"step {step}, n {n}, residual")
            else:
                pay = mx_sr.compress(host[i], fmt, keys[i], step, kind == "rht", ROT_KEY, half)
            P[i].expect(pay)
            P[i].check(f"step {step}, n {n}, payload")
            G[i].check(f"step {step}, n {n}, gradient")
    assert cache.built == 2                                     # one plan a (device, dtype)
    cache.close()


@pytest.mark.parametrize("divisor", [1, 3])
@pytest.mark.parametrize("nsrc", [1, 2, 9, 16])
@dtypes
@pytest.mark.parametrize("fmt, kind", [(f, k) for f in ("fp8", "fp4") for k in ("ef", "rht")])
def test_fold_many(fmt, kind, dt, nsrc, divisor):
    """The two folds (the unrotated stateless wires take the error-feedback
    wires').  Source 0 comes from a half-precision worker, the others from
    float32 workers; source 1 carries a non-finite block.  A float32 output
    rides in the same call."""
    rng = np.random.default_rng(nsrc * 4 + divisor)
    comp, tdt, step = COMP[fmt, kind], getattr(torch, dt), STEP
    ns, outs_dt = SIZES + [100], [dt] * len(SIZES) + [None]
    pays = []
    for n in ns:
        srcs = [values(rng, n, None, 6).astype(F) for s in range(nsrc)]
        g0, srcs[0] = half_input(dt, srcs[0])
        if nsrc > 1 and n > 40:
            srcs[1][40] = np.inf
        one = [mx_sr.compress(g, fmt, KEY + s, step, kind == "rht", ROT_KEY, False) if kind == "rht"
               else mx.compress(g, np.zeros(n, F), fmt)[0] for s, g in enumerate(srcs)]
        half = (mx_sr.compress(g0, fmt, KEY, step, True, ROT_KEY, dt == "bfloat16") if kind == "rht"
                else mx.compress(g0, np.zeros(n, F), fmt, dt == "bfloat16")[0])
        assert np.array_equal(half, one[0])
        pays.append(one)
    S = [[Buf(p) for p in one] for one in pays]
    O = [Buf(np.full(n * (2 if d else 4), 0x5A, np.uint8), (0, 2, 4, 8)[i % 4] if d else 0)
         for i, (n, d) in enumerate(zip(ns, outs_dt))]
    outs = [o.view(tdt if d else torch.float32) for o, d in zip(O, outs_dt)]
    lists = [[b.view() for b in row] for row in S]
    if kind == "rht":
        comp.fold_many_into(outs, lists, divisor, [ROT_KEY] * len(ns), step)
    else:
        comp.fold_many_into(outs, lists, divisor)
    torch.cuda.synchronize()
    for i, (n, d) in enumerate(zip(ns, outs_dt)):
        O[i].expect(define_fold(pays[i], n, fmt, kind, divisor, d))
        O[i].check(f"n {n}, output")
