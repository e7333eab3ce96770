"""The server round of the top-k wire on the host:
topk.refold is compress(fold(...)), the order of the sum and the tie rule show
in its bytes, push_pull of topk_ef.at(ratio) contexts through an opt-in
ServerFrontend's packed store on numpy payloads equals the numpy model byte for
byte, the store tells top-k keys from the other wires whatever their k, and the
refold plan's operand checks run with no GPU."""
import threading

import numpy as np
import pytest

from prophet_amd import reducer, topk
from prophet_amd.buckets import cantor_command
from prophet_amd.compression import Compression
from prophet_amd.pushpull import K_COMPRESSED_PUSH_PULL, ServerFrontend, Worker

F = np.float32
TK = Compression.topk_ef.at(0.25)


class Stub:
    """No element-wise server: a packed context never reaches it."""


def payload(n, idx, val):
    """A payload of the entries (idx, val), the header as compress writes it."""
    head = np.array([len(idx), n, 0, 0], "<u4")
    return np.concatenate([head, np.asarray(idx, "<u4"),
                           np.asarray(val, "<f4").view("<u4")]).view(np.uint8)


def host_round(grads, cuts, nw, ratio):
    """The model of `grads[t][w]` over partitions `cuts`: per worker and
    partition compress, the server's refold, the one-source fold with the
    divisor.  Returns (outputs and pulled payloads per round, the workers'
    residuals, the server's)."""
    n = grads[0][0].size
    want, pulled = [], []
    wres, sres = [np.zeros(n, F) for _ in range(nw)], np.zeros(n, F)
    for t in range(len(grads)):
        want.append(np.empty(n, F))
        pulled.append([])
        for lo, hi in cuts:
            k = topk.k_for(hi - lo, ratio)
            ps = []
            for w in range(nw):
                p, wres[w][lo:hi] = topk.compress(grads[t][w][lo:hi], wres[w][lo:hi], k)
                ps.append(p)
            p, sres[lo:hi] = topk.refold(ps, hi - lo, sres[lo:hi], k)
            want[t][lo:hi] = topk.fold([p], hi - lo, nw, k)
            pulled[t].append(p)
    return want, pulled, wres, sres


def test_refold_is_the_composition():
    n, k = 8, 2
    ps = [payload(n, [1, 5], [3.0, -1.0]), payload(n, [5, 6], [1.0, 0.5]),
          payload(n, [0, 1], [0.25, -3.5])]
    res = np.array([0, 0.125, 4, 0, 0, 0, -0.5, np.nan], F)
    p, r = topk.refold(ps, n, res)                      # k from the payloads' size
    wp, wr = topk.compress(topk.fold(ps, n, 1, k), res, k)
    assert p.tobytes() == wp.tobytes() and r.tobytes() == wr.tobytes()
    # c = [0.25, -0.375, 4, 0, 0, 0, 0, NaN]: the NaN's key is the largest, then 4
    assert p.tobytes() == payload(n, [2, 7], [4.0, np.nan]).tobytes()
    assert r.tobytes() == np.array([0.25, -0.375, 0, 0, 0, 0, 0, 0], F).tobytes()
    for wrap in (np.asarray, lambda a: pytest.importorskip("torch").from_numpy(a)):
        out, rr = wrap(np.zeros(p.size, np.uint8)), wrap(res.copy())
        TK.refold_many_into([out], [rr], [[wrap(x.copy()) for x in ps]])
        assert np.asarray(out).tobytes() == p.tobytes() and np.asarray(rr).tobytes() == r.tobytes()
    with pytest.raises(ValueError, match="1..16"):
        topk.refold(ps * 6, n, res)
    with pytest.raises(ValueError, match="differ in size"):
        TK.refold_many_into([np.zeros(16 + 8, np.uint8)], [res.copy()], [ps])


def test_the_order_of_the_sum_and_the_tie_rule():
    n, z = 4, np.zeros(4, F)
    a, b, c = (payload(n, [2], [v]) for v in (2.0 ** 24, 1.0, -2.0 ** 24))
    fwd, _ = topk.refold([a, b, c], n, z)               # (2^24 + 1) - 2^24 = 0: all keys tie
    rev, _ = topk.refold([a, c, b], n, z)               # (2^24 - 2^24) + 1 = 1
    assert fwd.tobytes() == payload(n, [0], [0.0]).tobytes()
    assert rev.tobytes() == payload(n, [2], [1.0]).tobytes()
    # sources that cancel to exact zero: the lowest indices win the tie
    p, r = topk.refold([payload(n, [1, 3], [5.0, -2.0]), payload(n, [1, 3], [-5.0, 2.0])], n, z)
    assert p.tobytes() == payload(n, [0, 1], [0.0, 0.0]).tobytes() and not r.any()


def test_round_on_numpy_payloads():
    nw, n, bound = 2, 300, 800                          # partitions of 200 and 100 elements
    fe = ServerFrontend(Stub(), size=nw, packed_wires=(TK,))
    rng = np.random.default_rng(7)
    grads = [[rng.standard_normal(n).astype(F) * F(w + 1) for w in range(nw)] for _ in range(2)]
    workers = [Worker(w, fe, partition_bytes=bound) for w in range(nw)]
    outs = [[None, None] for _ in range(nw)]
    pulled = [[None, None] for _ in range(nw)]

    def run(w):
        ctx = workers[w].init_tensor("g", np.zeros(n, F), 0, compression=TK)
        assert [ln for _, _, ln in ctx.parts] == [16 + 8 * 50, 16 + 8 * 25]
        for t in range(2):
            outs[w][t] = np.empty(n, F)
            workers[w].push_pull("g", grads[t][w].copy(), output=outs[w][t], average=True)
            pulled[w][t] = [ctx.staging[off:off + ln].tobytes() for _, off, ln in ctx.parts]

    threads = [threading.Thread(target=run, args=(w,)) for w in range(nw)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(100)
    assert not any(t.is_alive() for t in threads)
    want, stag, _, sres = host_round(grads, ((0, 200), (200, 300)), nw, TK.RATIO)
    for t in range(2):
        for w in range(nw):
            assert outs[w][t].tobytes() == want[t].tobytes(), (w, t)
            assert pulled[w][t] == [p.tobytes() for p in stag[t]], (w, t)
    got = np.concatenate([fe.packed.residual(k) for k in workers[0].contexts["g"].key_list])
    assert got.tobytes() == sres.tobytes()
    assert Compression.topk_ef.at(0.25) is TK and not TK.SERVER_ROUND


def test_store_tells_topk_keys_from_the_other_wires():
    """k == 4 and k == 8 are the block-scaled wires' first header words."""
    M8, M4 = Compression.mxfp8_ef, Compression.mxfp4_ef
    fe = ServerFrontend(Stub(), size=1, packed_wires=(M8, M4, TK))
    cmd = cantor_command(K_COMPRESSED_PUSH_PULL, 3)
    keys = {1: (TK, 16), 2: (TK, 32), 3: (M8, 64), 4: (M4, 64)}      # k_for(16) == 4, (32) == 8
    for key, (C, n) in keys.items():
        fe.push(cmd, key, 0, C.init_payload(n), C.payload_nbytes(n))
        assert fe.packed._keys[key].comp is C and fe.packed._keys[key].n == n
    assert topk.header(TK.init_payload(32)) == (8, 32)
    assert Compression.onebit_ef.init_payload(64)[12:16].view("<u4")[0] == 0
    bad = TK.init_payload(16)
    bad[0:4] = np.array([5], "<u4").view(np.uint8)      # k that does not match the size
    with pytest.raises(ValueError, match="top-k init payload"):
        fe.push(cmd, 9, 0, bad, bad.size)
    other = ServerFrontend(Stub(), size=1, packed_wires=(Compression.topk_ef.at(0.5),))
    with pytest.raises(ValueError, match="does not refold"):
        other.push(cmd, 9, 0, TK.init_payload(16), TK.payload_nbytes(16))
    with pytest.raises(ValueError, match="fold_many_into"):
        Worker(0, other).init_tensor("g", np.zeros(16, F), 0, compression=TK)


A, R, O, P = 0x10000, 0x20000, 0x30000, 0x40000
BAD = [
    ([([P], 0, O, 64, 4)], 1), ([([P], R, 0, 64, 4)], 1), ([([0], R, O, 64, 4)], 1),   # null
    ([([P], R, O, 64, 0)], 1), ([([P], R, O, 64, 65)], 1), ([([P], 0, O, 0, 1)], 1),   # k
    ([([P], R, O, (1 << 31) + 1, 4)], 1),
    ([([P + 8], R, O, 64, 4)], 1), ([([P], R, O + 4, 64, 4)], 1),                      # payloads
    ([([P], R + 2, O, 64, 4)], 1),                                                     # residual
    ([([P, P], R, O, 64, 4)], 2), ([([P, P + 32], R, O, 64, 4)], 2),                   # overlaps:
    ([([O + 16], R, O, 64, 4)], 1), ([([P], R, R + 240, 64, 4)], 1),                   # out, resid
    ([([R + 128], R, O, 64, 4)], 1),
    ([([P], R, O, 64, 4), ([P + 64], R + 0x1000, O + 32, 64, 4)], 1),                  # two outs
    ([([], R, O, 64, 4)], 0), ([([P + 64 * s for s in range(17)], R, O, 64, 4)], 17),  # nsrc
]


@pytest.mark.parametrize("segs,nsrc", BAD, ids=range(len(BAD)))
def test_operand_checks_run_before_any_device_call(segs, nsrc):
    with pytest.raises(reducer.ReduceError) as e:
        reducer.GpuReducer().topk_refold_plan(segs, nsrc)
    assert e.value.code == reducer.EARGS
