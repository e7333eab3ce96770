"""PowerSGD on the GPU: byteps_reduce_powersgd_*
(prophet_amd/csrc/bpsr_k_powersgd.hip) against prophet_amd/powersgd.py.

The projections run on matrix instructions in the kernels' own order and are
held to gamma_K (|M| @ |Q|), the bound of an f32 dot product of K terms in any
order; the ``g + R`` left in R, ``finish`` and determinism are byte for byte.
The shapes: one partial tile each way at rank 1; a convolution with n = 64 and
nine column chunks; m off a multiple of 4 (the element path) with 65 chunks;
rank 16 with n and m off every tile; ten row chunks in PROJECT-Q; and the first
two as the segments of one plan (a plan has one rank: 2, the largest at which
17 rows still are 8 r).  Inputs are standard normal."""
import functools
import threading

import numpy as np
import pytest

from prophet_amd import powersgd, reducer
from prophet_amd.compression import CastPlanCache, Compression

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

F, D, U = np.float32, np.float64, 2.0 ** -24
SHAPES = [(17, 37, 1), (64, 576, 4), (33, 4100, 3), (250, 515, 16), (300, 70, 2)]
PLANS = [[s] for s in SHAPES] + [[(17, 37, 2), (64, 576, 2)]]
IDS = ["-".join("x".join(map(str, s)) for s in p) for p in PLANS]


def gamma(k):
    return k * U / (1 - k * U)


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


class Seg:
    """One segment's operands on the device, from standard normals."""

    def __init__(self, rng, n, m, r):
        self.n, self.m, self.r = n, m, r
        self.host = {"g": rng.standard_normal((n, m)).astype(F),
                     "R": rng.standard_normal((n, m)).astype(F), "Q": powersgd.init_q(m, r, n + m)}
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")      # noqa: E731
        self.g, self.R, self.Q = (torch.from_numpy(self.host[k]).cuda() for k in "gRQ")
        self.P, self.Qn, self.out = z(n, r), z(m, r), z(n, m)

    def args(self):
        return (self.g, self.R, self.P, self.Q, self.Qn, self.out, self.n, self.m)


def run(plan, phase, segs, restore=()):
    """`phase` after putting `restore` = [(attribute, arrays)] back; returns
    every segment's R, P, Qn and out as numpy arrays."""
    for name, arrays in restore:
        for s, a in zip(segs, arrays):
            getattr(s, name).copy_(torch.from_numpy(a))
    getattr(plan, phase)()
    torch.cuda.synchronize()
    return {k: [getattr(s, k).cpu().numpy() for s in segs] for k in ("R", "P", "Qn", "out")}


@functools.lru_cache(maxsize=None)
def pipeline(which):
    """The four phases once over PLANS[which], each run twice from the same
    bytes; what every phase left, shared by the tests below."""
    assert torch.cuda.is_available()
    red = reducer.GpuReducer(device=0)
    rng = np.random.default_rng(which)
    segs = [Seg(rng, *s) for s in PLANS[which]]
    plan = red.powersgd_plan([s.args() for s in segs], segs[0].r)
    got, again = {}, {}
    got["p"] = run(plan, "project_p", segs)
    again["p"] = run(plan, "project_p", segs, [("R", [s.host["R"] for s in segs])])
    got["o"] = run(plan, "orthogonalize", segs)
    again["o"] = run(plan, "orthogonalize", segs, [("P", got["p"]["P"])])
    got["q"] = run(plan, "project_q", segs)
    again["q"] = run(plan, "project_q", segs)
    got["f"] = run(plan, "finish", segs)
    again["f"] = run(plan, "finish", segs, [("R", got["q"]["R"])])
    plan.close()
    return segs, got, again


CASES = pytest.mark.parametrize("which", range(len(PLANS)), ids=IDS)


@CASES
def test_projections_against_float64(which):
    segs, got, _ = pipeline(which)
    for i, s in enumerate(segs):
        M = s.host["g"] + s.host["R"]
        assert same(got["p"]["R"][i], M) and same(got["q"]["R"][i], M)
        M64, Q64 = M.astype(D), s.host["Q"].astype(D)
        err = np.abs(got["p"]["P"][i] - M64 @ Q64)
        bound = gamma(s.m) * (np.abs(M64) @ np.abs(Q64))
        print(f"P {s.n}x{s.m} r{s.r}: worst error / bound {(err / bound).max():.3f}")
        assert (err <= bound).all()
        Ph = got["o"]["P"][i].astype(D)
        err = np.abs(got["q"]["Qn"][i] - M64.T @ Ph)
        bound = gamma(s.n) * (np.abs(M64).T @ np.abs(Ph))
        print(f"Qn {s.n}x{s.m} r{s.r}: worst error / bound {(err / bound).max():.3f}")
        assert (err <= bound).all()


@CASES
def test_every_phase_is_deterministic(which):
    _, got, again = pipeline(which)
    for phase in "poqf":
        for k in ("R", "P", "Qn", "out"):
            assert all(same(a, b) for a, b in zip(got[phase][k], again[phase][k])), (phase, k)


@CASES
@pytest.mark.parametrize("poison", [False, True], ids=["finite", "inf"])
def test_finish_is_the_definition_byte_for_byte(which, poison):
    segs, got, _ = pipeline(which)
    if not poison:
        for i, s in enumerate(segs):
            R, out = got["q"]["R"][i].copy(), np.empty((s.n, s.m), F)
            powersgd.finish(out, R, got["o"]["P"][i], got["q"]["Qn"][i])
            assert same(got["f"]["out"][i], out) and same(got["f"]["R"][i], R)
        return
    # an inf in g reaches R through project_p; P and Qn are set apart from it
    red, rng = reducer.GpuReducer(device=0), np.random.default_rng(which)
    segs = [Seg(rng, s.n, s.m, s.r) for s in segs]
    for s in segs:
        s.g[s.n // 2, s.m - 1] = float("inf")
        s.g[0, 0] = float("-inf")
    plan = red.powersgd_plan([s.args() for s in segs], segs[0].r)
    M = run(plan, "project_p", segs)["R"]
    P = [rng.standard_normal((s.n, s.r)).astype(F) for s in segs]
    Qn = [rng.standard_normal((s.m, s.r)).astype(F) for s in segs]
    fin = run(plan, "finish", segs, [("P", P), ("Qn", Qn)])
    plan.close()
    for i, s in enumerate(segs):
        assert np.isinf(M[i][0, 0]) and np.isinf(M[i][s.n // 2, s.m - 1])
        R, out = M[i].copy(), np.empty((s.n, s.m), F)
        powersgd.finish(out, R, P[i], Qn[i])
        assert same(fin["out"][i], out) and same(fin["R"][i], R)
        assert R[0, 0] == 0 and R[s.n // 2, s.m - 1] == 0 and np.isfinite(fin["R"][i]).all()


@CASES
def test_orthogonalize_against_the_float64_lines(which):
    """On n x r Gaussians, n >= 8 r.  The tolerance: 16 times the error the
    definition's own float32 evaluation shows against float64 on these inputs."""
    red, rng = reducer.GpuReducer(device=0), np.random.default_rng(100 + which)
    segs = [Seg(rng, *s) for s in PLANS[which]]
    plan = red.powersgd_plan([s.args() for s in segs], segs[0].r)
    P = [rng.standard_normal((s.n, s.r)).astype(F) for s in segs]
    got = run(plan, "orthogonalize", segs, [("P", P)])["P"]
    holed = [p.copy() for p in P]
    for p in holed:
        p[:, -1] = 0
    zeroed = run(plan, "orthogonalize", segs, [("P", holed)])["P"]
    plan.close()
    for i, s in enumerate(segs):
        assert s.n >= 8 * s.r
        want = powersgd.orthogonalize(P[i].astype(D), dtype=D)
        host = np.abs(powersgd.orthogonalize(P[i].copy()) - want).max()
        dev = np.abs(got[i] - want).max()
        print(f"orthogonalize {s.n}x{s.r}: host f32 error {host:.3e}, device error {dev:.3e}")
        assert host > 0 and dev <= 16 * host
        assert np.abs(got[i].astype(D).T @ got[i].astype(D) - np.eye(s.r)).max() <= 16 * host
        assert not zeroed[i][:, -1].any() and np.isfinite(zeroed[i]).all()


def host_round(grads, rank, dtype):
    """`powersgd.py` over every worker's gradients of the compressing tensor,
    P and Qn averaged: the outs, per iteration."""
    nw, (n, m) = len(grads[0]), grads[0][0].shape
    R, Q, outs = [np.zeros((n, m), dtype) for _ in range(nw)], powersgd.init_q(m, rank, 0).astype(dtype), []
    for gs in grads:
        P = sum(powersgd.project_p(g, r, Q, dtype=dtype) for g, r in zip(gs, R)) / dtype(nw)
        powersgd.orthogonalize(P, dtype=dtype)
        Q = sum(powersgd.project_q(r, P, dtype=dtype) for r in R) / dtype(nw)
        for r in R:
            out = powersgd.finish(np.empty((n, m), dtype), r, P, Q, dtype=dtype)
        outs.append(out)
    return outs


def test_the_round_over_a_server():
    """Two workers, a compressing 64 x 64 x 3 x 3 tensor and a pass-through
    bias, two iterations."""
    from prophet_amd.pushpull import ServerFrontend, Worker
    from prophet_amd.server import PSServer
    assert torch.cuda.is_available()
    N, ITERS, RANK = 2, 2, 4
    rng = np.random.default_rng(7)
    grads = [[rng.standard_normal((64, 576)).astype(F) for _ in range(N)] for _ in range(ITERS)]
    bias = [[rng.standard_normal(64).astype(F) for _ in range(N)] for _ in range(ITERS)]
    srv = PSServer(N)
    fe = ServerFrontend(srv)
    workers = [Worker(r, fe, partition_bytes=64 << 10) for r in range(N)]
    seen, errors = {}, []

    def work(w):
        try:
            with torch.cuda.device(0):
                named = {"w": torch.zeros(64, 64, 3, 3, device="cuda"),
                         "b": torch.zeros(64, device="cuda")}
                states, plans = powersgd.make_states(named, RANK), CastPlanCache(4)
                assert states["b"] is None and states["w"].P.shape == (64, RANK)
                for it in range(ITERS):
                    named["w"].copy_(torch.from_numpy(grads[it][w.rank]).view(64, 64, 3, 3))
                    named["b"].copy_(torch.from_numpy(bias[it][w.rank]))
                    M = grads[it][w.rank] + states["w"].R.cpu().numpy()
                    powersgd.push_pull_many(w, named, states, average=True, plans=plans)
                    torch.cuda.synchronize()
                    seen[(w.rank, it)] = (named["w"].cpu().numpy().reshape(64, 576), M,
                                          states["w"].R.cpu().numpy(), states["w"].Q.cpu().numpy(),
                                          named["b"].cpu().numpy())
                assert plans.built == 2                      # Q and Qn change places
                plans.close()
        except Exception as e:  # surfaced below
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(w,)) for w in workers]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=100)
    for w in workers:
        w.close()
    srv.close()
    assert not errors, errors
    o32, o64 = host_round(grads, RANK, F), host_round(grads, RANK, D)
    for it in range(ITERS):
        (out, M, R, Q, b), other = seen[(0, it)], seen[(1, it)]
        assert same(out, other[0]) and same(Q, other[3]) and same(b, other[4])
        assert same(b, (bias[it][0] + bias[it][1]) / F(N))
        for o, m, r, _, _ in (seen[(0, it)], other):
            assert same(r, np.where(np.isfinite(o) & np.isfinite(m), m - o, F(0)))
        host, dev = np.abs(o32[it] - o64[it]).max(), np.abs(out - o64[it]).max()
        print(f"round, iteration {it}: host f32 error {host:.3e}, device error {dev:.3e}")
        assert host > 0 and dev <= 16 * host
