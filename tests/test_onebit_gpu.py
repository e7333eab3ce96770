"""1-bit sign compression with error feedback on the GPU:
byteps_reduce_onebit_* (prophet_amd/csrc/bpsr_k_onebit.hip) against
prophet_amd/onebit.py, byte for byte.

Sizes: every path of the kernels — one element, a ragged word, whole words, a
word and one element, around a b128 vector, around the 4,096-element tile, and
three full tiles + 5 words + 37 elements — as plans of one segment and of all
sizes together, with the float32 operands 16-byte aligned (vector paths) and
4 bytes off (element paths).  Every operand lies between 0xA5 bytes, and the
whole buffers are compared.

Inputs of kind (a) are multiples of 2^-10 below 4 in magnitude (negative zero,
exact zeros and both signs in every word among them): their f64 sum is exact
in any order (tests/test_onebit.py), so the scale and every byte are pinned.
Their mean is about 2, so the scale is a multiple of 2^-24, every new residual
too, and the second step's |c| (below 16, at most 2^42 such units in all) is of
kind (a) again.  Inputs of kind (b) are general: the scale may differ from
math.fsum's by one float32 neighbour (the f64 sum's (n-1) 2^-53 relative error,
then one rounding), and everything else is pinned given the header's scale."""
import numpy as np
import pytest

from prophet_amd import onebit, reducer

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TILE = 4096
SIZES = [1, 63, 64, 65, 255, 256, TILE - 1, TILE, TILE + 1, 3 * TILE + 64 * 5 + 37]
PLANS = [[n] for n in SIZES] + [SIZES]
PAD, SENT = 256, 0xA5


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


def exact_inputs(rng, n):
    q = np.float32(2.0 ** -10)
    g = rng.integers(-4096, 4097, n).astype(np.float32) * q
    r = rng.integers(-64, 65, n).astype(np.float32) * q
    g[0], r[0] = 3.0, 0.25
    if n > 8:
        g[1], r[1] = -0.0, -0.0               # c = -0.0: not negative
        g[2], r[2] = 1.5, -1.5                # c = +0.0
        g[5::64], g[6::64] = 2.0, -2.0        # both signs in every word
    return g, r


def compress_case(red, sizes, off, make, scale_from_header):
    rng = np.random.default_rng(len(sizes) * 8 + off)
    host = [make(rng, n) for n in sizes]
    G = [Buf(g, off) for g, _ in host]
    R = [Buf(r, off) for _, r in host]
    P = [Buf(np.full(onebit.payload_bytes(n), 0x5A, np.uint8)) for n in sizes]
    plan = red.onebit_plan([(g.view(torch.float32), r.view(torch.float32), p.view(), n)
                            for g, r, p, n in zip(G, R, P, sizes)])
    res = [r for _, r in host]
    for step in range(2):
        plan.compress()
        torch.cuda.synchronize()
        for i, n in enumerate(sizes):
            scale = None
            if scale_from_header:
                scale = onebit.header(P[i].view().cpu().numpy())[0]
                ref = onebit.mean_abs(host[i][0] + res[i])
                assert scale in (np.nextafter(ref, np.float32(-np.inf)), ref,
                                 np.nextafter(ref, np.float32(np.inf))), (n, scale, ref)
            pay, res[i] = onebit.compress(host[i][0], res[i], scale)
            P[i].expect(pay)
            R[i].expect(res[i])
            for b, name in ((P[i], "payload"), (R[i], "residual"), (G[i], "gradient")):
                b.check(f"step {step}, n {n}, {name}")
    plan.close()


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("sizes", PLANS, ids=lambda s: "all" if len(s) > 1 else str(s[0]))
def test_compress_exact_inputs_two_steps(red, sizes, off):
    compress_case(red, sizes, off, exact_inputs, scale_from_header=False)


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("sizes", PLANS, ids=lambda s: "all" if len(s) > 1 else str(s[0]))
def test_compress_general_inputs(red, sizes, off):
    def general(rng, n):
        mag = np.float32(2.0) ** rng.integers(-12, 8, n).astype(np.float32)
        return (rng.standard_normal(n).astype(np.float32) * mag,
                rng.standard_normal(n).astype(np.float32) * np.float32(0.1))
    compress_case(red, sizes, off, general, scale_from_header=True)


def fold_payload(rng, n, scale):
    """A payload with random bits and a header whose count is not n: the fold
    takes its sizes from the plan."""
    p, _ = onebit.compress(rng.standard_normal(n).astype(np.float32), np.zeros(n, np.float32))
    p[0:4] = np.array([scale], dtype="<f4").view(np.uint8)
    p[4:12] = 0xFF
    return p


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("sizes", PLANS, ids=lambda s: "all" if len(s) > 1 else str(s[0]))
def test_fold(red, sizes, nsrc, divisor, off):
    rng = np.random.default_rng(nsrc * 16 + divisor + off)
    # +-2^24 absorbs a +-1 that comes after it and not one that came before
    scales = [2.0 ** 24, 1.0, 2.0 ** 24, 0.75, 1.0, 3.0, 2.0 ** 24, 1.0] * 2
    host = [[fold_payload(rng, n, scales[k]) for k in range(nsrc)] for n in sizes]
    P = [[Buf(p) for p in ps] for ps in host]
    O = [Buf(np.full(n, np.nan, np.float32), off) for n in sizes]
    plan = red.onebit_fold_plan([(o.view(torch.float32), [p.view() for p in ps], n)
                                 for o, ps, n in zip(O, P, sizes)], nsrc)
    plan.launch(divisor)
    torch.cuda.synchronize()
    plan.close()
    for o, ps, bufs, n in zip(O, host, P, sizes):
        o.expect(onebit.fold(ps, n, divisor))
        o.check(f"n {n}, output")
        for b in bufs:
            b.check(f"n {n}, payload")


def test_refused_calls_leave_every_byte(red):
    n = TILE + 65
    g, r = exact_inputs(np.random.default_rng(1), n)
    G, R, O = Buf(g), Buf(r), Buf(np.zeros(n, np.float32))
    P = [Buf(fold_payload(np.random.default_rng(k), n, 1.0)) for k in range(2)]
    gv, rv, ov = (b.view(torch.float32) for b in (G, R, O))
    pv = [p.view() for p in P]
    odd = P[0].dev[P[0].lo + 8:P[0].hi - 8]          # a payload 8 bytes off
    for segs in ([(0, rv, pv[0], n)], [(gv, 0, pv[0], n)], [(gv, rv, 0, n)],
                 [(gv, rv, odd, n - 128)], [(gv, gv[64:], pv[0], n - 64)],
                 [(gv, rv, pv[0], n), (ov, gv, pv[1], n)]):
        with pytest.raises(reducer.ReduceError) as e:
            red.onebit_plan(segs)
        assert e.value.code == reducer.EARGS
    for segs, nsrc in (([(0, pv, n)], 2), ([(ov, [pv[0], 0], n)], 2),
                       ([(ov, [odd], n - 128)], 1), ([(ov, [], n)], 0),
                       ([(ov, pv * 9, n)], 18), ([(ov, [pv[0], pv[0]], n)], 2),
                       ([(ov, [pv[0], ov.view(torch.uint8)[:pv[0].numel()]], n)], 2)):
        with pytest.raises(reducer.ReduceError) as e:
            red.onebit_fold_plan(segs, nsrc)
        assert e.value.code == reducer.EARGS
    comp = red.onebit_plan([(gv, rv, pv[0], n)])
    fold = red.onebit_fold_plan([(ov, [pv[1]], n)], 1)
    lib = red.lib
    assert lib.byteps_reduce_onebit_fold_plan_launch(comp.handle, 1, None) == reducer.EARGS
    assert lib.byteps_reduce_onebit_plan_compress(fold.handle, None) == reducer.EARGS
    for d in (0, -1):
        assert lib.byteps_reduce_onebit_fold_plan_launch(fold.handle, d, None) == reducer.EARGS
    torch.cuda.synchronize()
    comp.close()
    fold.close()
    for b in [G, R, O] + P:
        b.check("a refused call")
