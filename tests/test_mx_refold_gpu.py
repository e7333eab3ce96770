"""The server round of the block-scaled error-feedback wires on the GPU
(DESIGN.md §11.17): byteps_reduce_mx_refold_* (prophet_amd/csrc/
bpsr_k_mx_refold.hip) against prophet_amd/mx.py's refold, byte for byte — there
is no tolerance in the scheme — and push_pull of mxfp8_ef / mxfp4_ef device
tensors through an opt-in ServerFrontend's packed store.

One plan holds every size of test_mx_gpu's SIZES and an empty segment: around a
b128 vector, a block of 32, the 4,096-element tile and a ragged fp4 tail.  Every
operand lies between 0xA5 bytes and whole buffers are compared; two launches a
plan, so a residual the device wrote feeds the next."""
import numpy as np
import pytest

from prophet_amd import mx, reducer
from test_mx import COMP, FMTS
from test_mx_gpu import SIZES, TILE, Buf, fold_sources, make_inputs
from test_mx_refold import host_round, run_workers

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

F = np.float32


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return reducer.GpuReducer(device=0)


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("nsrc", [1, 2, 9, 16])         # 9: one past a group of 8
@pytest.mark.parametrize("fmt", FMTS)
def test_refold_two_launches(red, fmt, nsrc, off):
    rng = np.random.default_rng(nsrc * 8 + off)
    shape = SIZES + [0]
    srcs = [fold_sources(rng, n, nsrc, fmt) for n in shape]
    res = [make_inputs("scaled", rng, n, fmt)[1] for n in shape]
    for ps, r, n in zip(srcs, res, shape):
        if n >= 96:
            # block 2: source 0 scaled up to 2^125 at its largest code, the residual near
            # FLT_MAX with each element's sign, so that c = sum + r overflows
            ps[0][16 + 2] = 244 if fmt == "fp8" else 250
            r[64:96] = np.copysign(F(3.0e38), mx.decode(ps[0], n, fmt)[64:96])
    S = [[Buf(p) for p in ps] for ps in srcs]
    R = [Buf(r, off) for r in res]
    O = [Buf(np.full(mx.payload_bytes(n, fmt), 0x5A, np.uint8)) for n in shape]
    plan = red.mx_refold_plan([([p.view() for p in ps], r.view(torch.float32), o.view(), n)
                               for ps, r, o, n in zip(S, R, O, shape)], nsrc, fmt)
    for step in range(2):
        plan.launch()
        torch.cuda.synchronize()
        for i, n in enumerate(shape):
            pay, res[i] = mx.refold(srcs[i], n, res[i], fmt)
            O[i].expect(pay)
            R[i].expect(res[i])
            for b, name in [(O[i], "output payload"), (R[i], "residual")] + \
                    [(s, "source") for s in S[i]]:
                b.check(f"step {step}, n {n}, {name}")
    plan.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_refused_calls_leave_every_byte(red, fmt):
    n = TILE + 1
    rng = np.random.default_rng(1)
    R = Buf(np.ones(n, F))
    P = [Buf(p) for p in fold_sources(rng, n, 3, fmt)]
    rv, pv = R.view(torch.float32), [p.view() for p in P]
    odd = P[0].dev[P[0].lo + 8:P[0].hi - 8]              # a payload 8 bytes off
    for segs, nsrc in (([(pv[:1] * 17, rv, pv[2], n)], 17),            # a 17th source
                       ([([pv[0]], rv, pv[0], n)], 1),                 # out is a source
                       ([([odd], rv, pv[2], n - 128)], 1),             # a misaligned source
                       ([([pv[0]], rv, odd, n - 128)], 1)):            # a misaligned output
        with pytest.raises((reducer.ReduceError, ValueError)) as e:
            red.mx_refold_plan(segs, nsrc, fmt)
        assert getattr(e.value, "code", reducer.EARGS) == reducer.EARGS
    fold = red.mx_fold_plan([(rv, [pv[1]], n)], 1, fmt)
    lib = red.lib
    assert lib.byteps_reduce_mx_refold_plan_launch(None, None) == reducer.EARGS   # a null plan
    assert lib.byteps_reduce_mx_refold_plan_launch(fold.handle, None) == reducer.EARGS
    torch.cuda.synchronize()
    fold.close()
    for b in [R] + P:
        b.check("a refused call")


@pytest.mark.parametrize("fmt", FMTS)
def test_two_workers_two_rounds_through_the_frontend(fmt):
    """Device tensors through the opt-in front end, push_pull and
    push_pull_iteration, equal the host model's bytes."""
    from prophet_amd.pushpull import ServerFrontend, Worker
    C, nw, n, bound = COMP[fmt], 2, 4396, 16408          # partitions of 4,102 and 294 elements
    rng = np.random.default_rng(7)
    grads = [[rng.standard_normal(n).astype(F) * F(w + 1) for w in range(nw)] for _ in range(2)]
    want, wres, sres = host_round(grads, [(0, 4102), (4102, n)], nw, fmt)
    for mode in ("push_pull", "iteration"):
        fe = ServerFrontend(object(), size=nw, packed_wires=(C,))
        workers = [Worker(w, fe, partition_bytes=bound) for w in range(nw)]
        outs = [[None, None] for _ in range(nw)]

        def run(w):
            torch.cuda.set_device(0)
            workers[w].init_tensor("g", torch.zeros(n, device="cuda"), 0, compression=C)
            for t in range(2):
                g = torch.from_numpy(grads[t][w]).cuda()
                if mode == "push_pull":
                    workers[w].push_pull("g", g, average=True)
                else:
                    workers[w].push_pull_iteration({"g": g}, average=True)
                outs[w][t] = g.cpu().numpy()

        run_workers(nw, run)
        for w in range(nw):
            assert [o.tobytes() for o in outs[w]] == [x.tobytes() for x in want], (mode, w)
            assert workers[w].residual("g").cpu().numpy().tobytes() == wres[w].tobytes()
        keys = workers[0].contexts["g"].key_list
        assert torch.cat([fe.packed.residual(k) for k in keys]).cpu().numpy().tobytes() == \
            sres.tobytes()
        for wk in workers:
            wk.close()
        fe.packed.close()
