"""The server round of the block-scaled error-feedback wires on the host
(DESIGN.md §11.17): mx.refold is compress(fold(...)), the device-free
refold_many_into equals it, and push_pull of mxfp8_ef / mxfp4_ef contexts
through an opt-in ServerFrontend's packed store on numpy payloads equals the
numpy model byte for byte — the scheme has no floating reduction."""
import threading

import numpy as np
import pytest

from prophet_amd import mx, onebit
from prophet_amd.buckets import cantor_command
from prophet_amd.compression import Compression
from prophet_amd.pushpull import K_COMPRESSED_PUSH_PULL, ServerFrontend, Worker

torch = pytest.importorskip("torch")

F = np.float32
FMTS = ["fp8", "fp4"]
COMP = {"fp8": Compression.mxfp8_ef, "fp4": Compression.mxfp4_ef}


class Stub:
    """No element-wise server: a packed context never reaches it."""


def sources(rng, n, nsrc, fmt):
    """`nsrc` payloads; source 1 carries an X == 255 block."""
    gs = [rng.standard_normal(n).astype(F) * F(2.0 ** s) for s in range(nsrc)]
    if nsrc > 1:
        gs[1][40] = np.inf
    return [mx.compress(g, np.zeros(n, F), fmt)[0] for g in gs]


def run_workers(nw, body):
    threads = [threading.Thread(target=body, args=(w,)) for w in range(nw)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(100)
    assert not any(t.is_alive() for t in threads)


def host_round(grads, cuts, nw, fmt):
    """The model of `grads[t][w]` over partitions `cuts`: per worker and
    partition compress, the server's refold, the one-source fold with the
    divisor.  Returns (outputs per round, workers' residuals, the server's)."""
    n = grads[0][0].size
    want, wres, sres = [], [np.zeros(n, F) for _ in range(nw)], np.zeros(n, F)
    for t in range(len(grads)):
        want.append(np.empty(n, F))
        for lo, hi in cuts:
            ps = []
            for w in range(nw):
                p, wres[w][lo:hi] = mx.compress(grads[t][w][lo:hi], wres[w][lo:hi], fmt)
                ps.append(p)
            p, sres[lo:hi] = mx.refold(ps, hi - lo, sres[lo:hi], fmt)
            want[t][lo:hi] = mx.fold([p], hi - lo, fmt, nw)
    return want, wres, sres


@pytest.mark.parametrize("nsrc", [1, 3])
@pytest.mark.parametrize("fmt", FMTS)
def test_refold_is_the_composition(fmt, nsrc):
    n, rng = 77, np.random.default_rng(nsrc)
    ps, res = sources(rng, n, nsrc, fmt), rng.standard_normal(n).astype(F)
    p, r = mx.refold(ps, n, res, fmt)
    wp, wr = mx.compress(mx.fold(ps, n, fmt), res, fmt)
    assert p.tobytes() == wp.tobytes() and r.tobytes() == wr.tobytes()
    assert mx.header(p) == (mx.bits_of(fmt), n) and p.size == mx.payload_bytes(n, fmt)
    if nsrc > 1:                                       # the bad block: X 255, codes 0, r' the NaN
        assert p[16 + 1] == 255 and (r[32:64].view(np.uint32) == 0x7fc00000).all()
    # the device-free refold_many_into: numpy and CPU tensors, the residual in place
    for wrap in (np.asarray, torch.from_numpy):
        out, rr = wrap(np.zeros(p.size, np.uint8)), wrap(res.copy())
        COMP[fmt].refold_many_into([out], [rr], [[wrap(x.copy()) for x in ps]])
        assert np.asarray(out).tobytes() == p.tobytes() and np.asarray(rr).tobytes() == r.tobytes()
    with pytest.raises(ValueError, match="1..16"):
        mx.refold(ps * 17, n, res, fmt)
    with pytest.raises(ValueError, match="1..16"):
        COMP[fmt].refold_many_into([p], [res], [list(ps) * 17])


@pytest.mark.parametrize("nw", [2, 3])
@pytest.mark.parametrize("fmt", FMTS)
def test_round_on_numpy_payloads(fmt, nw):
    C, n, bound = COMP[fmt], 300, 800                  # partitions of 200 and 100 elements
    fe = ServerFrontend(Stub(), size=nw, packed_wires=(C,))
    rng = np.random.default_rng(nw)
    grads = [[rng.standard_normal(n).astype(F) * F(w + 1) for w in range(nw)] for _ in range(2)]
    workers = [Worker(w, fe, partition_bytes=bound) for w in range(nw)]
    outs = [[None, None] for _ in range(nw)]

    def run(w):
        ctx = workers[w].init_tensor("g", np.zeros(n, F), 0, compression=C)
        assert [ln for _, _, ln in ctx.parts] == [mx.payload_bytes(200, fmt),
                                                  mx.payload_bytes(100, fmt)]
        for t in range(2):
            outs[w][t] = np.empty(n, F)
            workers[w].push_pull("g", grads[t][w].copy(), output=outs[w][t], average=True)

    run_workers(nw, run)
    want, wres, sres = host_round(grads, ((0, 200), (200, 300)), nw, fmt)
    for w in range(nw):
        assert [o.tobytes() for o in outs[w]] == [x.tobytes() for x in want], w
        assert workers[w].residual("g").tobytes() == wres[w].tobytes()
    got = np.concatenate([fe.packed.residual(k) for k in workers[0].contexts["g"].key_list])
    assert got.tobytes() == sres.tobytes()


@pytest.mark.parametrize("fmt", FMTS)
def test_the_round_is_opt_in(fmt):
    C = COMP[fmt]
    other = COMP["fp4" if fmt == "fp8" else "fp8"]
    for wires in ((), (other,)):
        fe = ServerFrontend(Stub(), size=1, packed_wires=wires)
        with pytest.raises(ValueError, match="fold_many_into"):
            Worker(0, fe).init_tensor("g", np.zeros(8, F), 0, compression=C)
        # the store itself refuses a key of a wire its front end does not name
        with pytest.raises(ValueError, match="does not refold"):
            fe.push(cantor_command(K_COMPRESSED_PUSH_PULL, 3), 7, 0, C.init_payload(8),
                    C.payload_nbytes(8))
    with pytest.raises(ValueError, match="float32"):
        Worker(0, ServerFrontend(Stub(), size=1, packed_wires=(C,))).init_tensor(
            "g", np.zeros(8, np.float16), 2, compression=C)


def test_one_front_end_carries_both_wires_in_one_iteration():
    C, OB, n = Compression.mxfp8_ef, Compression.onebit_ef, 100
    fe = ServerFrontend(Stub(), size=1, packed_wires=(C,))
    wk = Worker(0, fe)
    rng = np.random.default_rng(0)
    g = {"a": rng.standard_normal(n).astype(F), "b": rng.standard_normal(n).astype(F)}
    wk.init_tensor("a", np.zeros(n, F), 0, compression=OB)
    wk.init_tensor("b", np.zeros(n, F), 0, compression=C)
    t = {k: v.copy() for k, v in g.items()}
    wk.push_pull_iteration(t)
    z = np.zeros(n, F)
    pa = onebit.refold([onebit.compress(g["a"], z)[0]], n, z)[0]
    pb = mx.refold([mx.compress(g["b"], z, "fp8")[0]], n, z, "fp8")[0]
    assert t["a"].tobytes() == onebit.fold([pa], n, 1).tobytes()
    assert t["b"].tobytes() == mx.fold([pb], n, "fp8").tobytes()
