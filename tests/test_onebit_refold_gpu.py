"""The server round of the 1-bit wire on the GPU:
byteps_reduce_onebit_refold_* (prophet_amd/csrc/bpsr_k_onebit_refold.hip)
against prophet_amd/onebit.py's refold, byte for byte, and push_pull of
Compression.onebit_ef device tensors through ServerFrontend's packed store.

Sizes: one element, around a word, around a wave's 1,024 elements, around the
4,096-element tile, three tiles + 5 words + 37; one segment a plan and all in
one plan; the residual 16-byte aligned and 4 bytes off; every operand between
0xA5 bytes, whole buffers compared, two launches so the residual carries.

Inputs of kind (a): source scales 2^24 and 1 (2^24 absorbs a 1 that comes after
it, so the fold's order shows) and residuals that are multiples of 0.25 below
16.  Every |c| of the first step is a multiple of 0.25 below 2^29: under 2^45
units in all.  Source 0's scale is 2^24, so about half the elements or more
hold a sum of 2^24 or above and the first scale is an integer; the new
residuals are then multiples of 0.25 again, below 2^30, and the second step's
total stays under 2^46 units (on the host model with these seeds the largest
total of either step is 2^41 units of its smallest bit).  Below 2^53 units the
f64 sum is exact in any order, so every byte of both steps is pinned.  General
inputs pin the header's scale to one float32 neighbour of math.fsum's and all
else given it."""
import threading

import numpy as np
import pytest

from prophet_amd import onebit, reducer
from prophet_amd.compression import Compression
from prophet_amd.pushpull import ServerFrontend, Worker

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

TILE = 4096
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 3 * TILE + 64 * 5 + 37]
PLANS = [[n] for n in SIZES] + [SIZES]
PAD, SENT = 256, 0xA5
SCALES = [2.0 ** 24, 1.0, 2.0 ** 24, 1.0, 1.0, 1.0, 2.0 ** 24, 1.0] * 2


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return reducer.GpuReducer(device=0)


class Buf:
    """`data` on the device at 16-byte alignment + `off`, between PAD sentinel
    bytes; `want` is the host image to compare with."""

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
        bad = np.flatnonzero(self.dev.cpu().numpy() != self.want)
        assert bad.size == 0, f"{what}: first differing byte {bad[0] - self.lo} of the operand"


def source(rng, n, scale):
    """A payload with random bits and a header whose count is not n: sizes
    come from the plan."""
    p, _ = onebit.compress(rng.standard_normal(n).astype(np.float32), np.zeros(n, np.float32))
    p[0:4] = np.array([scale], dtype="<f4").view(np.uint8)
    p[4:12] = 0xFF
    return p


def near(scale, ref):
    return scale in (np.nextafter(ref, np.float32(-np.inf)), ref,
                     np.nextafter(ref, np.float32(np.inf)))


def refold_case(red, sizes, nsrc, off, general):
    rng = np.random.default_rng(len(sizes) * 64 + nsrc * 2 + off // 4)
    scales = list(rng.uniform(0.5, 3.0, nsrc)) if general else SCALES
    host = [[source(rng, n, scales[k]) for k in range(nsrc)] for n in sizes]
    res = [(rng.standard_normal(n) if general else rng.integers(-63, 64, n) * 0.25)
           .astype(np.float32) for n in sizes]
    S = [[Buf(p) for p in ps] for ps in host]
    R = [Buf(r, off) for r in res]
    O = [Buf(np.full(onebit.payload_bytes(n), 0x5A, np.uint8)) for n in sizes]
    plan = red.onebit_refold_plan([([p.view() for p in ps], r.view(torch.float32), o.view(), n)
                                   for ps, r, o, n in zip(S, R, O, sizes)], nsrc)
    for step in range(2):
        plan.launch()
        torch.cuda.synchronize()
        for i, n in enumerate(sizes):
            scale = None
            if general:
                scale = onebit.header(O[i].view().cpu().numpy())[0]
                ref = onebit.mean_abs(onebit.fold(host[i], n, 1) + res[i])
                assert near(scale, ref), (n, scale, ref)
            pay, res[i] = onebit.refold(host[i], n, res[i], scale)
            O[i].expect(pay)
            R[i].expect(res[i])
            for b, name in [(O[i], "output payload"), (R[i], "residual")] + \
                    [(s, "source") for s in S[i]]:
                b.check(f"step {step}, n {n}, {name}")
    plan.close()


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("nsrc", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("sizes", PLANS, ids=lambda s: "all" if len(s) > 1 else str(s[0]))
def test_refold_exact_inputs_two_steps(red, sizes, nsrc, off):
    refold_case(red, sizes, nsrc, off, general=False)


def test_refold_general_inputs(red):
    refold_case(red, SIZES, 3, 0, general=True)


def test_refused_calls_leave_every_byte(red):
    n = TILE + 65
    rng = np.random.default_rng(1)
    R, G = Buf(np.ones(n, np.float32)), Buf(np.ones(n, np.float32))
    P = [Buf(source(rng, n, 1.0)) for _ in range(3)]
    rv, gv = R.view(torch.float32), G.view(torch.float32)
    pv = [p.view() for p in P]
    odd = P[0].dev[P[0].lo + 8:P[0].hi - 8]          # a payload 8 bytes off
    for segs, nsrc in (([([0, pv[1]], rv, pv[2], n)], 2), ([(pv[:2], 0, pv[2], n)], 2),
                       ([(pv[:2], rv, 0, n)], 2), ([([odd], rv, pv[2], n - 128)], 1),
                       ([([pv[0]], rv, odd, n - 128)], 1), ([([], rv, pv[2], n)], 0),
                       ([(pv[:1] * 17, rv, pv[2], n)], 17), ([([pv[0], pv[0]], rv, pv[2], n)], 2),
                       ([([pv[0]], rv, pv[0], n)], 1), ([([pv[0]], rv, pv[2], (1 << 37) + 1)], 1),
                       ([([rv.view(torch.uint8)[:pv[0].numel()]], rv, pv[2], n)], 1),
                       ([([pv[0]], rv, pv[2], n), ([pv[1]], gv, pv[2], n)], 1)):
        with pytest.raises((reducer.ReduceError, ValueError)) as e:
            red.onebit_refold_plan(segs, nsrc)
        assert getattr(e.value, "code", reducer.EARGS) == reducer.EARGS
    refold = red.onebit_refold_plan([([pv[0]], rv, pv[2], n)], 1)
    comp = red.onebit_plan([(gv, rv, pv[2], n)])
    fold = red.onebit_fold_plan([(gv, [pv[1]], n)], 1)
    lib = red.lib
    assert lib.byteps_reduce_onebit_refold_plan_launch(comp.handle, None) == reducer.EARGS
    assert lib.byteps_reduce_onebit_refold_plan_launch(fold.handle, None) == reducer.EARGS
    assert lib.byteps_reduce_onebit_refold_plan_launch(None, None) == reducer.EARGS
    assert lib.byteps_reduce_onebit_plan_compress(refold.handle, None) == reducer.EARGS
    assert lib.byteps_reduce_onebit_fold_plan_launch(refold.handle, 1, None) == reducer.EARGS
    torch.cuda.synchronize()
    for p in (refold, comp, fold):
        p.close()
    for b in [R, G] + P:
        b.check("a refused call")


def test_two_workers_two_rounds_through_the_frontend():
    """Worker w's gradient is +-2^w throughout: its scale is exact and its
    residual returns to zero, so round 1 is pinned byte for byte and round 2
    given the scale the server wrote."""
    nw, n, bound = 2, 4396, 16408                     # partitions of 4,102 and 294 elements
    cuts = [(0, 4102), (4102, n)]
    rng = np.random.default_rng(7)
    grads = [[np.where(rng.integers(0, 2, n) > 0, 1.0, -1.0).astype(np.float32) *
              np.float32(2.0 ** w) for w in range(nw)] for _ in range(2)]
    got = {}
    for mode in ("push_pull", "iteration"):
        fe = ServerFrontend(object(), size=nw)
        workers = [Worker(w, fe, partition_bytes=bound) for w in range(nw)]
        outs = [[None, None] for _ in range(nw)]
        pulled = [[None, None] for _ in range(nw)]

        def run(w):
            torch.cuda.set_device(0)
            wk = workers[w]
            ctx = wk.init_tensor("g", torch.zeros(n, device="cuda"), 0,
                                 compression=Compression.onebit_ef)
            for t in range(2):
                g = torch.from_numpy(grads[t][w]).cuda()
                if mode == "push_pull":
                    wk.push_pull("g", g, average=True)
                else:
                    wk.push_pull_iteration({"g": g}, average=True)
                outs[w][t], pulled[w][t] = g.cpu().numpy(), ctx.staging.cpu().numpy()

        threads = [threading.Thread(target=run, args=(w,)) for w in range(nw)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(100)
        assert not any(t.is_alive() for t in threads)
        sres = np.zeros(n, np.float32)
        for t in range(2):
            want, at = np.empty(n, np.float32), 0
            for lo, hi in cuts:
                ps = [onebit.compress(grads[t][w][lo:hi], np.zeros(hi - lo, np.float32))[0]
                      for w in range(nw)]
                scale = None
                if t == 1:
                    scale = onebit.header(pulled[0][t][at:at + 16])[0]
                    assert near(scale, onebit.mean_abs(onebit.fold(ps, hi - lo, 1) + sres[lo:hi]))
                p, sres[lo:hi] = onebit.refold(ps, hi - lo, sres[lo:hi], scale)
                want[lo:hi] = onebit.fold([p], hi - lo, nw)
                for w in range(nw):
                    assert pulled[w][t][at:at + p.size].tobytes() == p.tobytes(), (mode, t, w, lo)
                at += (p.size + 15) & ~15
            for w in range(nw):
                assert outs[w][t].tobytes() == want.tobytes(), (mode, t, w)
        for w in range(nw):
            assert not workers[w].residual("g").cpu().numpy().any()
        keys = workers[0].contexts["g"].key_list
        assert torch.cat([fe.packed.residual(k) for k in keys]).cpu().numpy().tobytes() == \
            sres.tobytes()
        got[mode] = (outs, pulled)
        for wk in workers:
            wk.close()
        fe.packed.close()
    for w in range(nw):
        for t in range(2):
            for a, b in zip(got["push_pull"], got["iteration"]):
                assert a[w][t].tobytes() == b[w][t].tobytes()
