"""The server's keyed consumer (blockq_key_kernel) at the tile sizes, queue
widths, dtypes and cache policies no other server test runs, bit for bit
against the oracle's left fold in the chosen arrival order.

The consumer instantiates the tile cores with arguments of its own: up to 8
workers fold_tile_full_buf / fold_tile_body with NS = -8 (eight pointers
permuted in registers) and a NaN replay through PermSrcs, 9 to 16 workers
NS = 0 and PermSrcs16 with the block's second release word; key_tile_done
counts a tile once its stores have drained — at once for full tiles of a
write-through launch, after an agent release fence and a second drain under
the plain and nt policies.  tests/test_server_order_gpu.py runs all of that at
VPT 1 (a tile of 256 x 16 B, where a replay that re-read slot 0 or a wrong
valid[j] cannot show), fp32 once at VPT 2 without a partial tile, floats only
and write-through only.

Here: the keys of tests/server_shapes.py — 1 element, 7 elements, one full
tile + 1 element, and 3 full tiles + a partial tile (300 vectors at VPT 2:
slot 1 valid on lanes 0..43; 700 at VPT 4: slot 2 on lanes 0..187, slot 3
nowhere) + a ragged tail — with BPSR_BQ_VPT set before the server is created,
order_probe's probes in every slot of the first, the interior and the last
full tile, the partial tile and the tail (tests/test_server_shapes.py shows on
the CPU that a slot-0 replay, slot order, a dropped second word and a dropped
slot change bytes there), integer dtypes on synth's ``bits``.  Driving and
checks are test_server_order_gpu's: device releases, an init round, 3
slot-written rounds in order_probe.round_order's orders with data of their
own, key_info's order the chosen one, every key pulled N times a round as
device view, blocking device copy and host copy in turn — while the consumer
kernel is still resident, from a store the previous round's pulls have read.
Every case asserts from stats() that it ran the tile size, tile count and
cache policy it names.

Policies: write-through (every table below 96 MiB); plain through
set_tuning(nt=0); nt, which a server takes from 96 MiB of keys of one dtype
on, in one fresh child process with BPSR_WT_MAX_MIB=0 (the threshold is read
once a process): this file run as a script."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import fold_shapes as fs  # noqa: E402
import server_shapes as ss  # noqa: E402
from test_server_order_gpu import KEYS, Rig, slot_rounds  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]


@pytest.fixture(scope="module")
def port():
    from oracle.oracle import PortReducer
    assert torch.cuda.is_available()
    return PortReducer(nthreads=4)


@pytest.fixture(scope="module")
def red():
    from prophet_amd.reducer import GpuReducer
    return GpuReducer(device=0)


@pytest.fixture
def plain(red):
    """Plain loads and stores for the launches of one test."""
    saved = red.get_tuning()
    try:
        red.set_tuning(nt=0)
        assert red.get_tuning()[1] == 0
        yield
    finally:
        red.set_tuning(*saved)
        assert red.get_tuning() == saved


def check_case(red, port, case, policy):
    """One server under device releases (BPSR_SERVER_RELEASE and BPSR_BQ_VPT
    set by the caller): the rounds, then the consumer's telemetry."""
    N, dt, vpt = case
    assert os.environ["BPSR_SERVER_RELEASE"] == "device"
    assert os.environ["BPSR_BQ_VPT"] == str(vpt)
    rig = Rig(red, port, dt, N, ss.inputs_of(dt, N, vpt), range(1, ss.ROUNDS + 1), engine_lanes=2)
    try:
        assert rig.srv.stats()["keyed_tiles"] == 0          # no queue yet
        st0, st = slot_rounds(rig, ss.ROUNDS)
    finally:
        rig.srv.close()
    assert st["consumer_launches"] == ss.ROUNDS, st
    assert st["key_releases"] == ss.ROUNDS * len(KEYS), st
    assert st["fold_launches"] == st0["fold_launches"], (st0, st)
    assert st["keyed_vpt"] == vpt, st
    assert st["keyed_tiles"] == ss.table_tiles(dt, vpt), st
    assert st["keyed_policy"] == policy, st


@pytest.mark.parametrize("case", ss.WT, ids=ss.case_id)
def test_keyed_consumer_write_through(red, port, case, monkeypatch):
    """Narrow queue (register path, PermSrcs replay), wide queue (PermSrcs16)
    and the integer instantiations, at the VPT of the case."""
    monkeypatch.setenv("BPSR_SERVER_RELEASE", "device")
    monkeypatch.setenv("BPSR_BQ_VPT", str(case[2]))
    check_case(red, port, case, fs.POL_WT)


@pytest.mark.parametrize("case", ss.PLAIN, ids=ss.case_id)
def test_keyed_consumer_plain(red, port, plain, case, monkeypatch):
    """kPolPlain: every tile takes key_tile_done's release fence and second
    drain before it is counted, and the pulls read what plain stores left."""
    monkeypatch.setenv("BPSR_SERVER_RELEASE", "device")
    monkeypatch.setenv("BPSR_BQ_VPT", str(case[2]))
    check_case(red, port, case, fs.POL_PLAIN)


@pytest.mark.timeout(240)
def test_keyed_consumer_nt_in_a_child_process():
    """One child with BPSR_WT_MAX_MIB=0 (no other environment touched): every
    case of server_shapes.NT prints its line."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)],
                       env=dict(os.environ, BPSR_WT_MAX_MIB="0"), cwd=ROOT,
                       capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for case in ss.NT:
        assert f"nt case passed: {ss.case_id(case)}" in r.stdout, r.stdout[-2000:]


if __name__ == "__main__":
    assert os.environ.get("BPSR_WT_MAX_MIB") == "0"
    from oracle.oracle import PortReducer
    from prophet_amd.reducer import GpuReducer
    assert torch.cuda.is_available()
    _red, _port = GpuReducer(device=0), PortReducer(nthreads=4)
    assert _red.get_tuning()[1] == 1
    os.environ["BPSR_SERVER_RELEASE"] = "device"
    for _case in ss.NT:
        os.environ["BPSR_BQ_VPT"] = str(_case[2])
        check_case(_red, _port, _case, fs.POL_NT)
        print(f"nt case passed: {ss.case_id(_case)}", flush=True)
