"""The server round of the 1-bit wire on the host:
onebit.refold against compress(fold(...)) on hand-written vectors, and
push_pull of Compression.onebit_ef contexts through ServerFrontend's packed
store on numpy payloads, byte for byte against the numpy model (both sides sum
with math.fsum, so any input is exact)."""
import threading

import numpy as np
import pytest

from prophet_amd import onebit
from prophet_amd.buckets import cantor_command
from prophet_amd.compression import Compression
from prophet_amd.pushpull import K_COMPRESSED_PUSH_PULL, ServerFrontend, SgdStep, Worker

OB = Compression.onebit_ef


def f32(*xs):
    return np.array(xs, dtype=np.float32)


def test_refold_on_hand_written_vectors():
    pa = onebit.compress(f32(-2.0, 2.0, -2.0, 2.0), np.zeros(4, np.float32))[0]   # scale 2
    pb = onebit.compress(f32(2.0, -2.0, -2.0, 2.0), np.zeros(4, np.float32))[0]
    # the fold is (0, 0, -4, 4); c = (-0.0, +0.0, -3, 3): neither zero is negative
    p, r = onebit.refold([pa, pb], 4, f32(-0.0, 0.0, 1.0, -1.0))
    assert onebit.header(p) == (np.float32(1.5), 4) and p[16] == 0b0100
    assert r.tobytes() == f32(-1.5, -1.5, -1.5, 1.5).tobytes()
    # a NaN scale poisons the sum, the server's scale and every residual
    pn = pa.copy()
    pn[0:4] = f32(np.nan).view(np.uint8)
    p, r = onebit.refold([pa, pn], 4, np.zeros(4, np.float32))
    assert np.isnan(onebit.header(p)[0]) and not p[16:].any() and np.isnan(r).all()
    for n in (0, 1, 64, 65):
        rng = np.random.default_rng(n)
        ps = [onebit.compress(rng.standard_normal(n).astype(np.float32),
                              np.zeros(n, np.float32))[0] for _ in range(3)]
        res = rng.standard_normal(n).astype(np.float32)
        p, r = onebit.refold(ps, n, res)
        wp, wr = onebit.compress(onebit.fold(ps, n, 1), res)
        assert p.tobytes() == wp.tobytes() and r.tobytes() == wr.tobytes()
        assert p.size == onebit.payload_bytes(n)
        if n % 64:                                    # the pad bits are zero
            assert int(p[16:].view("<u8")[-1]) >> (n % 64) == 0


class Stub:
    """No element-wise server: a packed context never reaches it."""


@pytest.mark.parametrize("nw", [2, 3])
def test_round_on_numpy_payloads(nw):
    n, bound = 300, 800                                # partitions of 200 and 100 elements
    fe = ServerFrontend(Stub(), size=nw)
    rng = np.random.default_rng(nw)
    grads = [[rng.standard_normal(n).astype(np.float32) * np.float32(w + 1) for w in range(nw)]
             for _ in range(2)]
    workers = [Worker(w, fe, partition_bytes=bound) for w in range(nw)]
    outs = [[None, None] for _ in range(nw)]

    def run(w):
        wk = workers[w]
        ctx = wk.init_tensor("g", np.zeros(n, np.float32), 0, compression=OB)
        assert [ln for _, _, ln in ctx.parts] == [onebit.payload_bytes(200),
                                                  onebit.payload_bytes(100)]
        for t in range(2):
            outs[w][t] = np.empty(n, np.float32)
            wk.push_pull("g", grads[t][w].copy(), output=outs[w][t], average=True)

    threads = [threading.Thread(target=run, args=(w,)) for w in range(nw)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not any(t.is_alive() for t in threads)
    # the model: per worker and partition compress, the server's refold, the
    # one-source fold with the divisor
    wres = [np.zeros(n, np.float32) for _ in range(nw)]
    sres = np.zeros(n, np.float32)
    for t in range(2):
        want = np.empty(n, np.float32)
        for lo, hi in ((0, 200), (200, 300)):
            ps = []
            for w in range(nw):
                p, wres[w][lo:hi] = onebit.compress(grads[t][w][lo:hi], wres[w][lo:hi])
                ps.append(p)
            p, sres[lo:hi] = onebit.refold(ps, hi - lo, sres[lo:hi])
            want[lo:hi] = onebit.fold([p], hi - lo, nw)
        for w in range(nw):
            assert outs[w][t].tobytes() == want.tobytes(), (t, w)
    for w in range(nw):
        assert workers[w].residual("g").tobytes() == wres[w].tobytes()
    keys = workers[0].contexts["g"].key_list
    got = np.concatenate([fe.packed.residual(k) for k in keys])
    assert got.tobytes() == sres.tobytes()


def test_refusals():
    zero = np.zeros(onebit.payload_bytes(8), np.uint8)
    zero[4] = 8
    with pytest.raises(ValueError, match="request type 1"):
        ServerFrontend(Stub(), size=1).push(cantor_command(1, 3), 0, 0, zero, zero.size)
    with pytest.raises(ValueError, match="worker count"):
        ServerFrontend(Stub()).push(cantor_command(K_COMPRESSED_PUSH_PULL, 3), 0, 0, zero,
                                    zero.size)
    fe = ServerFrontend(Stub(), size=1)
    w = Worker(0, fe)
    w.init_tensor("g", np.zeros(8, np.float32), 0, compression=OB)
    key = w.contexts["g"].key_list[0]
    cmd = cantor_command(K_COMPRESSED_PUSH_PULL, 3)
    with pytest.raises(ValueError, match="bytes"):
        fe.push(cmd, key, 0, np.zeros(32, np.uint8), 32)          # a wrong payload size
    fe2 = ServerFrontend(Stub(), size=2)
    threads = [threading.Thread(target=fe2.push, args=(cmd, 7, r, zero, zero.size))
               for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    fe2.push(cmd, 7, 0, zero, zero.size)
    with pytest.raises(ValueError, match="twice"):
        fe2.push(cmd, 7, 0, zero, zero.size)                      # a double push
    g = {"g": np.ones(8, np.float32)}
    with pytest.raises(ValueError, match="stats"):
        w.push_pull("g", g["g"], stats=True)
    for kw in ({"stats": True}, {"clip_norm": 1.0},
               {"apply": SgdStep({"g": np.ones(8, np.float32)}, lr=0.1)}):
        with pytest.raises(ValueError, match="element-wise wire"):
            w.push_pull_iteration(g, **kw)
    assert not w.residual("g").any() and fe.packed.residual(key) is None    # nothing was pushed
