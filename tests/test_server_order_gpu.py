"""The server's folds on the order probes of tests/order_probe.py: every pull
equals, on the raw bytes, the oracle's left fold in the arrival order that
key_info reports — and that order is the one the test chose.

The probes (NaNs with a payload per worker, inf / -inf clashes, -0,
subnormals, +-(largest finite), at every third element of each tile region and
at every element of the ragged tails) send vectors to the exact replay
(fold_vector_exact) on every server path.  In the keyed consumer
(blockq_key_kernel) the fast path and the replay take the arrival order from
two pieces of code: up to 8 workers the fast path folds eight pointers
permuted in registers while the replay and the element work index the
record's pointer array through PermSrcs; 9 to 16 workers go through
PermSrcs16, positions 8..15 from the block's second release word.  A replay in
slot order, a dropped second word or element work that ignored the order
changes bytes here (tests/test_order_probe.py shows it on the CPU).

Driving, as test_server_gpu.test_device_release_epoch_launched_ahead_and_retired:
all device work on one non-default stream, stream syncs only, an init round of
blocking pushes from N threads, then every round from ONE thread — per key the
next order of order_probe.round_order, and for each worker in that order: copy
its bytes into recv_slot, synchronise the stream, push_ready.  So the arrival
order is chosen, not raced.

Keys (elements): 1, 7, one tile + 1, and 3 tiles + 100 vectors + 5 / 3 / 1
ragged elements (a tile at these sizes: 256 x 16 B, VPT 1)."""
import os
import threading

import numpy as np
import pytest

import order_probe as op
from oracle.oracle import PortReducer
from prophet_amd.dtypes import DType, elem_size

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

KEYS = [61, 62, 63, 64]


@pytest.fixture(scope="module")
def port():
    assert torch.cuda.is_available()
    return PortReducer(nthreads=4)


@pytest.fixture(scope="module")
def red():
    from prophet_amd.reducer import GpuReducer
    return GpuReducer(device=0)


class Rig:
    """One server, its stream, and the rounds' inputs: inputs_of(rnd, j) gives
    (per-worker bytes, probe kinds) of key number j."""

    def __init__(self, red, port, dt, N, inputs_of, rounds, **server_args):
        from prophet_amd.server import PSServer
        self.red, self.port, self.dt, self.N = red, port, dt, N
        self.inputs_of = inputs_of
        self.dev = torch.device("cuda:0")
        self.st = torch.cuda.Stream(device=self.dev)    # never the legacy NULL stream (server.h)
        self.lens = [len(inputs_of(1, j)[0][0]) for j in range(len(KEYS))]
        with torch.cuda.stream(self.st):
            self.src = {(r, j): [torch.from_numpy(x).to(self.dev) for x in inputs_of(r, j)[0]]
                        for r in rounds for j in range(len(KEYS))}
            self.zero = [torch.zeros(n, dtype=torch.uint8, device=self.dev) for n in self.lens]
        self.st.synchronize()
        self.srv = PSServer(N, **server_args)

    def on_stream(self, fn, *args):
        """For a thread of its own: the rig's stream, then the call."""
        torch.cuda.set_stream(self.st)
        fn(*args)

    def init_round(self):
        for j, k in enumerate(KEYS):
            ts = [threading.Thread(target=self.on_stream,
                                   args=(self.srv.push, k, w, self.zero[j], self.dt))
                  for w in range(self.N)]
            for t in ts:
                t.start()
            for t in ts:
                t.join(timeout=60)
                assert not t.is_alive()

    def slot_round(self, rnd, order_of):
        """The transport writes the slots: worker by worker in the chosen order."""
        for j, k in enumerate(KEYS):
            for w in order_of(j):
                x = self.src[(rnd, j)][w]
                self.red.copy(self.srv.recv_slot(k, w), x, x.numel(), stream=self.st)
                self.st.synchronize()
                self.srv.push_ready(k, w)

    def pushed_round(self, rnd, order_of, push):
        """Copied pushes in the chosen order, each from a thread started in
        that order (a push that waited would not hold the others back)."""
        ts = []
        for j, k in enumerate(KEYS):
            for w in order_of(j):
                t = threading.Thread(target=self.on_stream,
                                     args=(push, k, w, self.src[(rnd, j)][w], self.dt))
                t.start()
                t.join(timeout=5)
                ts.append(t)
        for t in ts:
            t.join(timeout=60)
            assert not t.is_alive()

    def pull_and_check(self, rnd, order_of, exact_order=True):
        """key_info's order is the chosen one; N pulls per key (the key re-arms
        after N), as device views, blocking device copies and host copies in
        turn, each equal to the oracle's fold in that order."""
        dt, N = self.dt, self.N
        for j, k in enumerate(KEYS):
            rounds, _, order = self.srv.key_info(k)
            assert rounds == rnd, (k, rounds)
            if exact_order:
                assert order == list(order_of(j)), (rnd, k, order)
            else:
                assert sorted(order) == list(range(N)), (rnd, k, order)
            ins, kind = self.inputs_of(rnd, j)
            n = self.lens[j]
            want = op.fold(self.port, dt, ins, order)
            for i in range(N):
                how = ("device view", "device copy", "host copy")[(i + rnd + j) % 3]
                if how == "device view":
                    p, ln = self.srv.pull_device_view(k)
                    assert ln == n
                    o = torch.empty(n, dtype=torch.uint8, device=self.dev)
                    self.red.copy(o, p, n, stream=self.st)
                    self.st.synchronize()
                    got = o.cpu().numpy()
                elif how == "device copy":
                    o = torch.empty(n, dtype=torch.uint8, device=self.dev)
                    self.srv.pull(k, o)
                    self.st.synchronize()
                    got = o.cpu().numpy()
                else:
                    got = np.zeros(n, np.uint8)
                    self.srv.pull(k, got)
                if not np.array_equal(got, want):
                    es = elem_size(dt)
                    m = n // es * es
                    U = np.dtype(f"u{es}")          # (integer dtypes too: server_shapes)
                    bad = (got[:m].view(U) != want[:m].view(U)).nonzero()[0]
                    raise AssertionError(
                        f"round {rnd} key {k} ({how}), order {order}: {len(bad)} of {m // es} "
                        "elements differ; first " + ", ".join(
                            f"[{e}] kind {int(kind[e])} got {int(got[:m].view(U)[e]):#x} "
                            f"want {int(want[:m].view(U)[e]):#x}" for e in bad[:6]))


def probe_inputs(dt, N):
    return lambda rnd, j: op.server_inputs(dt, N, rnd, j)


def slot_rounds(rig, rounds=op.ROUNDS):
    """`rounds` slot-written rounds in the orders of order_probe.round_order;
    returns the stats after round 1 and at the end."""
    st0 = None
    with torch.cuda.stream(rig.st):
        rig.init_round()
        for rnd in range(1, rounds + 1):
            order_of = lambda j, r=rnd: op.round_order(rig.N, r, j)   # noqa: E731
            rig.slot_round(rnd, order_of)
            rig.pull_and_check(rnd, order_of)
            if rnd == 1:
                st0 = rig.srv.stats()
    return st0, rig.srv.stats()


@pytest.mark.parametrize("case", op.DEVICE_NARROW + op.DEVICE_WIDE, ids=op.case_id)
def test_device_releases_fold_in_the_chosen_order(red, port, case, monkeypatch):
    """BPSR_SERVER_RELEASE=device, 3 rounds after the init round, one order
    each per key.  Up to 8 workers: the narrow queue (one release word; the
    fast path's registers against PermSrcs in the replay and the element
    work).  9 and 16 workers: the wide queue (PermSrcs16, positions 8..15 from
    the second release word).  The consumer folded every round: one consumer
    launch per round, every key released each round, no fold launch after
    round 1."""
    N, dt = case
    monkeypatch.setenv("BPSR_SERVER_RELEASE", "device")
    rig = Rig(red, port, dt, N, probe_inputs(dt, N), range(1, op.ROUNDS + 1), engine_lanes=2)
    try:
        st0, st = slot_rounds(rig)
    finally:
        rig.srv.close()
    assert st["consumer_launches"] == op.ROUNDS, st
    assert st["key_releases"] == op.ROUNDS * len(KEYS), st
    assert st["fold_launches"] == st0["fold_launches"], (st0, st)


def test_device_releases_one_real_tile_size(red, port, monkeypatch):
    """The tile size of a real table: 8 workers, fp32, the three small keys and
    one key of 16 MiB + 12 bytes.  build_table sums the keys' vectors (0 + 1 +
    256 + 2^20 = 1,048,833) and asks fold_vpt with the tuned VPT 2 of 8
    sources: ceil(1,048,833 / 512) = 2,049 tiles of 8 KiB per worker, not
    fewer than kMinTiles = 2,048, so VPT 2 stays (and 1,025 tiles of 16 KiB do
    not reach the mid-size VPT 4 rule, which starts at 2,048).  The big key is
    2,048 full tiles of 512 vectors and 3 tail elements; its probes lie in the
    first tile, the last full tile and the tail only, the rest is background.
    Reversed order, then — so that the fold launches can be compared after
    round 1, as everywhere — the same data once more in the rotated order."""
    dt, N = DType.FLOAT32, 8
    monkeypatch.setenv("BPSR_SERVER_RELEASE", "device")
    assert op.BIG_BYTES // 16 + (op.tile_elems(dt) + 1) // 4 + 7 // 4 == 1_048_833
    orders = op.orders(N)

    def inputs_of(rnd, j):
        return op.big_inputs(N) if j == 3 else op.server_inputs(dt, N, 1, j)

    rig = Rig(red, port, dt, N, inputs_of, [1], engine_lanes=2)
    rig.src.update({(2, j): rig.src[(1, j)] for j in range(len(KEYS))})
    assert rig.lens[3] == op.BIG_BYTES
    try:
        with torch.cuda.stream(rig.st):
            rig.init_round()
            for rnd in (1, 2):
                order_of = lambda j, r=rnd: orders[r - 1]      # noqa: E731
                rig.slot_round(rnd, order_of)
                rig.pull_and_check(rnd, order_of)
                if rnd == 1:
                    st0 = rig.srv.stats()
        st = rig.srv.stats()
    finally:
        rig.srv.close()
    assert st["consumer_launches"] == 2 and st["key_releases"] == 2 * len(KEYS), st
    assert st["fold_launches"] == st0["fold_launches"], (st0, st)


@pytest.mark.parametrize("policy", [0, 1], ids=["fused", "incremental"])
@pytest.mark.parametrize("case", op.LAUNCH, ids=op.case_id)
def test_launch_releases_fold_in_the_chosen_order(red, port, case, policy, monkeypatch):
    """BPSR_SERVER_RELEASE=launch: the lanes fold every round with launches
    (no consumer) — FUSED one batched fold per round (12 workers: the table
    path that reads the record's pointer array from memory), INCREMENTAL the
    in-place chain of sum(first arrival's slot, slot), where the replay
    re-reads an aliased srcs[0].  The same driving and checks."""
    N, dt = case
    monkeypatch.setenv("BPSR_SERVER_RELEASE", "launch")
    rig = Rig(red, port, dt, N, probe_inputs(dt, N), range(1, op.ROUNDS + 1), engine_lanes=2,
              policy=policy)
    try:
        st0, st = slot_rounds(rig)
    finally:
        rig.srv.close()
    assert st["consumer_launches"] == 0 and st["key_releases"] == 0, st
    assert st["fold_launches"] > st0["fold_launches"], (st0, st)      # the lanes folded


def test_copied_rounds_under_device_releases(red, port, monkeypatch):
    """Device releases, 8 workers, fp16: after one slot-written round (which
    builds the keyed queue) a round of blocking device pushes (landed by the
    copy service and released on the device: the consumer folds it) and a
    round of push_async (lane copies: it passes the consumer with a skip word
    and folds with a lane launch behind its copies), each issued in a chosen
    order.  The recorded order is checked as a permutation only; the bytes
    against the oracle in the recorded order."""
    N, dt = op.COPIED[0]
    monkeypatch.setenv("BPSR_SERVER_RELEASE", "device")
    rig = Rig(red, port, dt, N, probe_inputs(dt, N), range(1, 4), engine_lanes=2)
    stats = []
    try:
        with torch.cuda.stream(rig.st):
            rig.init_round()
            for rnd, push in ((1, None), (2, rig.srv.push), (3, rig.srv.push_async)):
                order_of = lambda j, r=rnd: op.round_order(N, r, j)   # noqa: E731
                if push is None:
                    rig.slot_round(rnd, order_of)
                else:
                    rig.pushed_round(rnd, order_of, push)
                rig.pull_and_check(rnd, order_of, exact_order=push is None)
                stats.append(rig.srv.stats())
    finally:
        rig.srv.close()
    service = os.environ.get("BPSR_SERVER_PULL_SERVICE", "1") != "0"
    assert stats[0]["key_releases"] == len(KEYS) and stats[0]["consumer_launches"] == 1, stats[0]
    if service:         # the blocking pushes: released on the device, no fold launch
        assert stats[1]["key_releases"] == 2 * len(KEYS), stats[1]
        assert stats[1]["fold_launches"] == stats[0]["fold_launches"], stats[:2]
    # push_async: lane launches, no device release
    assert stats[2]["fold_launches"] > stats[1]["fold_launches"], stats[1:]
    assert stats[2]["key_releases"] == stats[1]["key_releases"], stats[1:]
