"""The server round of the top-k wire on the GPU:
byteps_reduce_topk_refold_* (prophet_amd/csrc/bpsr_k_topk_refold.hip in front of
bpsr_k_topk.hip's select) against prophet_amd/topk.py's refold, byte for byte —
there is no tolerance in the scheme — and push_pull of topk_ef.at(ratio) device
tensors through an opt-in ServerFrontend's packed store.

Every operand lies between 0xA5 bytes and whole buffers are compared; two
launches a plan, so a residual the device wrote feeds the next.  Sizes go around
a b128 vector and the 4,096-element tile, k is 1, a middle value and n, the
residual 16-byte aligned (vector paths) and 4 bytes off (element paths).  From
the third source on, sources meet at elements 4095 and 4096 — the two sides of
a tile's edge — with 2^24, 1, -2^24, -1, so the sum there depends on the order
and cancels; source 0 and the residual carry a NaN, an inf and both zeros as
test_topk_gpu draws them."""
import numpy as np
import pytest

from prophet_amd import reducer, topk
from prophet_amd.compression import Compression
from test_topk_gpu import TILE, Buf, make_inputs
from test_topk_refold import host_round

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

F = np.float32
BIG = 2 * TILE + 5
# (segments of (n, k), nsrc, the residual's offset): every n, k of 1 / middle / n and nsrc
# at least once, 16 sources over several tiles, and one plan of many segments
CASES = [
    ([(1, 1)], 1, 0), ([(3, 2)], 2, 4), ([(4, 4)], 3, 0), ([(255, 1)], 8, 4),
    ([(TILE - 1, 2000)], 3, 0), ([(TILE, TILE)], 2, 4), ([(TILE + 1, 41)], 16, 0),
    ([(BIG, 300)], 16, 4), ([(BIG, BIG)], 3, 0), ([(BIG, 1)], 8, 0),
    ([(TILE + 1, 41), (0, 0), (BIG, 83), (3, 3), (255, 100)], 3, 4),
]


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return reducer.GpuReducer(device=0)


def sources(rng, n, k, nsrc):
    """`nsrc` payloads of k entries with garbage headers."""
    out = []
    for s in range(nsrc):
        want = [TILE - 1, TILE] if s >= 2 else [1, 3, 5, 6] if s == 0 and n > 8 else []
        forced = np.array([i for i in want if i < n][:k], np.int64)
        rest = rng.choice(np.setdiff1d(np.arange(n), forced), k - forced.size, replace=False)
        idx = np.sort(np.concatenate([forced, rest]))
        val = rng.integers(-8, 9, k).astype(F)
        if s >= 2:
            val[np.isin(idx, forced)] = [2.0 ** 24, 1.0, -2.0 ** 24, -1.0][(s - 2) % 4]
        for i, v in zip(forced if s == 0 else [], (np.nan, -np.inf, 0.0, -0.0)):
            val[idx == i] = v
        head = np.array([0xdeadbeef, 0xffffffff, 0x12345678, 0xa5a5a5a5], "<u4")
        out.append(np.concatenate([head, idx.astype("<u4"), val.view("<u4")]).view(np.uint8))
    return out


@pytest.mark.parametrize("shape,nsrc,off", CASES,
                         ids=[f"{'+'.join(f'{n}k{k}' for n, k in c[0])}-s{c[1]}-o{c[2]}"
                              for c in CASES])
def test_refold_two_rounds(red, shape, nsrc, off):
    rng = np.random.default_rng(len(shape) * 64 + nsrc * 2 + off)
    srcs = [sources(rng, n, k, nsrc) for n, k in shape]
    res = [make_inputs("general", rng, n)[1] for n, _ in shape]
    S = [[Buf(p) for p in ps] for ps in srcs]
    R = [Buf(r, off) for r in res]
    O = [Buf(np.full(topk.payload_bytes(k), 0x5A, np.uint8)) for _, k in shape]
    plan = red.topk_refold_plan([([p.view() for p in ps], r.view(torch.float32), o.view(), n, k)
                                 for ps, r, o, (n, k) in zip(S, R, O, shape)], nsrc)
    for step in range(2):
        plan.launch()
        torch.cuda.synchronize()
        for i, (n, k) in enumerate(shape):
            pay, res[i] = topk.refold(srcs[i], n, res[i], k)
            O[i].expect(pay)
            R[i].expect(res[i])
            for b, name in [(O[i], "output payload"), (R[i], "residual")] + \
                    [(s, "source") for s in S[i]]:
                b.check(f"step {step}, n {n}, k {k}, {name}")
    plan.close()


def test_refused_calls_leave_every_byte(red):
    n, k = TILE + 1, 41
    R = Buf(np.ones(n, F))
    P = [Buf(p) for p in sources(np.random.default_rng(1), n, k, 3)]
    rv, pv = R.view(torch.float32), [p.view() for p in P]
    odd = P[0].dev[P[0].lo + 8:P[0].hi - 8]              # a payload 8 bytes off
    for segs, nsrc in (([([pv[0]], rv, pv[0], n, k)], 1),              # out is a source
                       ([([odd], rv, pv[2], n, k - 2)], 1),            # a misaligned source
                       ([([pv[0]], rv, odd, n, k - 2)], 1)):           # a misaligned output
        with pytest.raises(reducer.ReduceError) as e:
            red.topk_refold_plan(segs, nsrc)
        assert e.value.code == reducer.EARGS
    fold = red.topk_fold_plan([(rv, [pv[1]], n, k)], 1)
    refold = red.topk_refold_plan([([pv[0]], rv, pv[2], n, k)], 1)
    lib = red.lib
    assert lib.byteps_reduce_topk_refold_plan_launch(None, None) == reducer.EARGS
    assert lib.byteps_reduce_topk_refold_plan_launch(fold.handle, None) == reducer.EARGS
    assert lib.byteps_reduce_topk_plan_compress(refold.handle, None) == reducer.EARGS
    assert lib.byteps_reduce_topk_fold_plan_launch(refold.handle, 1, None) == reducer.EARGS
    torch.cuda.synchronize()
    fold.close()
    refold.close()
    for b in [R] + P:
        b.check("a refused call")


def test_two_workers_two_rounds_through_the_frontend():
    """Device tensors through the opt-in front end, push_pull and
    push_pull_iteration, equal the host model's bytes."""
    import threading
    from prophet_amd.pushpull import ServerFrontend, Worker
    C, nw, n, bound = Compression.topk_ef.at(0.01), 2, 4396, 16408   # 4,102 and 294 elements
    rng = np.random.default_rng(7)
    grads = [[rng.standard_normal(n).astype(F) * F(w + 1) for w in range(nw)] for _ in range(2)]
    want, _, wres, sres = host_round(grads, [(0, 4102), (4102, n)], nw, C.RATIO)
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

        threads = [threading.Thread(target=run, args=(w,)) for w in range(nw)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(100)
        assert not any(t.is_alive() for t in threads)
        for w in range(nw):
            assert [o.tobytes() for o in outs[w]] == [x.tobytes() for x in want], (mode, w)
            assert workers[w].residual("g").cpu().numpy().tobytes() == wres[w].tobytes()
        keys = workers[0].contexts["g"].key_list
        assert torch.cat([fe.packed.residual(k) for k in keys]).cpu().numpy().tobytes() == \
            sres.tobytes()
        for wk in workers:
            wk.close()
        fe.packed.close()
