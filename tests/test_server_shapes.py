"""The keys and inputs of tests/server_shapes.py do what the keyed consumer's
GPU tests (tests/test_server_tiles_gpu.py) say they do.  No GPU.

Table shape: tests/cpp/fold_shapes.cpp — the unchanged bpsr_internal.h and
bpsr_table.cpp under g++ — builds every case's keyed table as keyq_create does
(one block per key, every key's sources in worker order, BPSR_BQ_VPT as
force_vpt) under the case's tuning; tile size, cache policy and tile count must
be the helper's, with full, partial and element records on the path the case
names (up to 8 workers the register path, above the pointer array).

Discriminating power, against the oracle alone, for every float case, round
and arrival order the GPU tests use: the model faults of blockq_key_kernel's
tile cores — a NaN replay that reads slot 0 for slot j, a replay or element
work in slot order, a dropped second release word, a partial tile whose last
valid slot is not written — each change bytes in every probed tile they
concern."""
import os
import subprocess

import numpy as np
import pytest

import fold_shapes as fs
import order_probe as op
import server_shapes as ss
from oracle.oracle import PortReducer
from prophet_amd.dtypes import DType, elem_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULT, PLAIN, NT = (1, -1), (0, -1), (1, 0)      # (nt, wt_max_mib; -1: the default 96)
POLICY_OF = {DEFAULT: fs.POL_WT, PLAIN: fs.POL_PLAIN, NT: fs.POL_NT}
CASES = ([(c, DEFAULT) for c in ss.WT] + [(c, PLAIN) for c in ss.PLAIN]
         + [(c, NT) for c in ss.NT])
FLOAT_CASES = list(dict.fromkeys(c for c, _ in CASES if ss.is_float(c[1])))
FULL_TILES = ("first_tile", "interior_tile", "last_full_tile")


@pytest.fixture(scope="module")
def port():
    return PortReducer(nthreads=1)


def ident(n):
    return list(range(n))


# -------------------------------------------------------------- table shape ----

def table_lines(case, tuning):
    N, dt, vpt = case
    lens = [n * elem_size(dt) for n in ss.key_elems(dt, vpt)]
    head = f"table {int(dt)} {tuning[0]} {tuning[1]} {vpt} {len(lens)} {len(lens)}"
    return [head] + [f"b {L} {N} {b} " + " ".join(["0"] * (N + 1)) for b, L in enumerate(lens)]


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = tmp_path_factory.mktemp("server_shapes") / "fold_shapes"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "prophet_amd", "csrc"),
                    os.path.join(ROOT, "prophet_amd", "csrc", "bpsr_table.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "fold_shapes.cpp"), "-o", str(exe)],
                   check=True)
    lines = [x for c in CASES for x in table_lines(*c)]
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    assert out[-1] == "done" and len(out) == len(CASES) + 1, out[-3:]
    got = []
    for x in out[:-1]:
        word, *fields = x.split()
        assert word == "table", x
        got.append({k: int(v) for k, v in (f.split("=") for f in fields)})
    return list(zip(CASES, got))


def test_every_case_gets_its_tile_size_policy_and_tile_count(tables):
    seen = set()
    for (case, tuning), got in tables:
        N, dt, vpt = case
        what = (ss.case_id(case), tuning)
        assert got["vpt"] == vpt and got["nmax"] == N, what
        assert got["pol"] == POLICY_OF[tuning], what
        assert got["tiles"] == ss.table_tiles(dt, vpt), what
        kinds = [ss.key_tiles(dt, vpt, j) for j in range(ss.NKEYS)]
        path, other = ("reg", "mem") if N <= 8 else ("mem", "reg")
        assert got["full_" + path] == sum(k["full"] for k in kinds), what
        assert got["partial_" + path] == sum(k["partial"] for k in kinds), what
        assert got["full_" + other] == 0 and got["partial_" + other] == 0, what
        assert got["elem"] == sum(k["elem"] for k in kinds) > 0, what
        # key 3: three full tiles and the partial one; key 2: one full tile
        assert kinds[ss.RAGGED] == {"elem": 1, "full": 3, "partial": 1}, what
        assert kinds[ss.ONE_TILE] == {"elem": 1, "full": 1, "partial": 0}, what
        assert kinds[0] == {"elem": 1, "full": 0, "partial": 0}, what
        seen.add((N > 8, int(dt), vpt, got["pol"]))
    # what the GPU file says it adds: both queues at VPT 2 and 4, 2-byte and
    # 8-byte types at VPT > 1, integers at VPT 1, 2 and 4, the other policies
    for wide in (False, True):
        for vpt in (2, 4):
            assert any(s[0] == wide and s[2] == vpt and s[3] == fs.POL_WT for s in seen)
        assert any(s[0] == wide and s[2] > 1 and elem_size(s[1]) == 2 for s in seen)
        assert any(s[0] == wide and s[2] > 1 and elem_size(s[1]) == 8 for s in seen)
    for vpt in (1, 2, 4):
        assert any(not ss.is_float(s[1]) and s[2] == vpt for s in seen), vpt
    for pol in (fs.POL_PLAIN, fs.POL_NT):
        assert any(s[3] == pol and s[2] == 1 for s in seen)
        assert any(s[3] == pol and s[2] > 1 and not s[0] for s in seen)
        assert any(s[3] == pol and s[2] > 1 and s[0] for s in seen)


def test_shapes_are_what_they_say():
    assert ss.slot_vecs(1) == [100] and ss.slot_vecs(2) == [256, 44]
    assert ss.slot_vecs(4) == [256, 256, 188, 0]
    for dt in (DType.FLOAT16, DType.BFLOAT16, DType.FLOAT32, DType.FLOAT64):
        assert ss.key_elems(dt, 1) == [n for n, _ in op.server_keys(dt)]
    for _, dt, vpt in dict.fromkeys(c for c, _ in CASES):
        n = ss.key_elems(dt, vpt)
        v = fs.vec_elems(dt)
        assert n[:2] == [1, 7] and n[2] == fs.K_BLOCK * vpt * v + 1
        nvec, tail_begin, body = fs.geometry(dt, n[3])
        assert nvec == 3 * fs.K_BLOCK * vpt + ss.PARTIAL_VECS[vpt]
        assert n[3] > tail_begin and n[3] * elem_size(dt) < 64 << 10
        reg = ss.key_regions(dt, vpt, ss.RAGGED)
        assert set(FULL_TILES + ("partial_tile",)) <= set(reg)
        assert "tail" in reg or "scalar_tail" in reg
        if DType(dt) == DType.FLOAT16:      # no element behind the vectors but the scalar tail
            assert "tail" not in reg and body == tail_begin
        assert set(ss.key_regions(dt, vpt, ss.ONE_TILE)) in ({"first_tile", "tail"},
                                                            {"first_tile", "scalar_tail"})


# ------------------------------------------------------ discriminating power ----

FLOATS = pytest.mark.parametrize("case", FLOAT_CASES, ids=ss.case_id)


def nan_vectors(dt, raw):
    """Per 16-byte vector of whole vectors `raw`: does it hold a NaN?"""
    return op.is_nan(dt, raw).reshape(-1, fs.vec_elems(dt)).any(axis=1)


def probed_tiles(dt, vpt, j):
    """[(name, element range)] of key j's probed tiles; every name must be
    there, so inputs without one of these regions fail here."""
    reg = ss.key_regions(dt, vpt, j)
    names = FULL_TILES + ("partial_tile",) if j == ss.RAGGED else ("first_tile",)
    return [(name, reg[name]) for name in names]


def rounds_of(port, case):
    """Per (round, key index in (2, 3)): sources, kinds, the order of the GPU
    test and the oracle's fold in it."""
    N, dt, vpt = case
    for rnd in range(1, ss.ROUNDS + 1):
        for j in (ss.ONE_TILE, ss.RAGGED):
            ins, kind = ss.inputs(dt, N, vpt, rnd, j)
            order = op.round_order(N, rnd, j)
            yield rnd, j, ins, kind, order, op.fold(port, dt, ins, order)


def tile_model(port, dt, ins, want, reg, vpt, src_slot, order):
    """The tile at `reg` as a kernel would write it whose fast path is right
    and whose NaN replay of slot j folds, in `order`, the lanes' vectors of
    slot src_slot(j) (whole vectors: for fp16 no scalar tail)."""
    es = elem_size(dt)
    lo0 = reg[0]
    tile = [np.ascontiguousarray(x[lo0 * es:reg[1] * es]).reshape(-1, 16) for x in ins]
    out = want[lo0 * es:reg[1] * es].copy()
    for j in range(vpt):
        lo, hi = fs.slot(dt, reg, j)
        if hi == lo:
            continue
        bad = nan_vectors(dt, want[lo * es:hi * es])
        if not bad.any():
            continue
        rows = [np.ascontiguousarray(x[src_slot(j) * fs.K_BLOCK:][:len(bad)][bad]).reshape(-1)
                for x in tile]
        sl = out[(lo - lo0) * es:(hi - lo0) * es].reshape(-1, 16)
        sl[bad] = op.fold(port, dt, rows, order).reshape(-1, 16)
    return out


@FLOATS
def test_every_slot_of_every_probed_tile_is_replayed_and_stored(port, case):
    """Every valid slot of every probed tile holds a vector whose result has
    a NaN (replayed); every slot of a probed full tile also one with none (the
    fast path's result is stored).  The partial tile's slots are valid where
    the GPU tests say."""
    N, dt, vpt = case
    es, v = elem_size(dt), fs.vec_elems(dt)
    for rnd, j, ins, kind, order, want in rounds_of(port, case):
        for name, reg in probed_tiles(dt, vpt, j):
            valid = []
            for s in range(vpt):
                lo, hi = fs.slot(dt, reg, s)
                valid.append((hi - lo) // v)
                if hi > lo:
                    nv = nan_vectors(dt, want[lo * es:hi * es])
                    assert nv.any(), (rnd, j, name, s)
                    if name != "partial_tile":
                        assert len(nv) == fs.K_BLOCK and not nv.all(), (rnd, j, name, s)
            if name == "partial_tile":
                assert valid == ss.slot_vecs(vpt), (rnd, valid)
        assert (kind[op.is_nan(dt, want)] >= 0).all()


@FLOATS
def test_replay_at_slot_0_changes_every_probed_tile(port, case):
    """The mutant fold_tile_full_buf / fold_tile_body whose replay of slot j
    re-reads the lane's slot-0 vector, in the arrival order: right at VPT 1,
    wrong bytes in every probed tile at VPT 2 and 4.  The model with the
    right slot is the oracle, so the mutation alone differs."""
    N, dt, vpt = case
    es = elem_size(dt)
    for rnd, j, ins, kind, order, want in rounds_of(port, case):
        for name, reg in probed_tiles(dt, vpt, j):
            ref = want[reg[0] * es:reg[1] * es]
            right = tile_model(port, dt, ins, want, reg, vpt, lambda s: s, order)
            assert np.array_equal(right, ref), (rnd, j, name)
            wrong = tile_model(port, dt, ins, want, reg, vpt, lambda s: 0, order)
            assert np.array_equal(wrong, ref) == (vpt == 1), (rnd, j, name)


@FLOATS
def test_slot_order_changes_every_probed_tile_and_the_element_work(port, case):
    """A replay in slot order 0..N-1 (the fast path right) changes bytes in
    every probed tile, and element work in slot order the elements behind the
    last whole vector, for every order that is not the identity (2 workers'
    third order is).  fp16 has no such element: its ragged elements are scalar
    tail, where no NaN names a worker; there the whole fold in slot order
    changes NaN-result probes of every tile."""
    N, dt, vpt = case
    es = elem_size(dt)
    for rnd, j, ins, kind, order, want in rounds_of(port, case):
        if order == ident(N):
            assert N == 2
            continue
        for name, reg in probed_tiles(dt, vpt, j):
            wrong = tile_model(port, dt, ins, want, reg, vpt, lambda s: s, ident(N))
            assert not np.array_equal(wrong, want[reg[0] * es:reg[1] * es]), (rnd, j, name)
        n = ss.key_elems(dt, vpt)[j]
        vt = op.vector_tail(dt, n)
        slot = op.fold(port, dt, ins, ident(N))
        d = op.changed(dt, want, slot)
        if DType(dt) == DType.FLOAT16:
            assert len(vt) == 0 and len(op.f16_scalar_tail(dt, n)) > 0
        else:
            assert len(vt) > 0 and (kind[vt.start:vt.stop] >= 0).all()
            assert d[vt.start:vt.stop].any(), (rnd, j)
        for name, (lo, hi) in probed_tiles(dt, vpt, j):
            assert (d & (kind >= 0) & op.is_nan(dt, want))[lo:hi].any(), (rnd, j, name)
    # the tiny keys: element work alone (fp16: scalar tail alone)
    if DType(dt) != DType.FLOAT16:
        for rnd in range(1, ss.ROUNDS + 1):
            for j in (0, 1):
                order = op.round_order(N, rnd, j)
                ins, _ = ss.inputs(dt, N, vpt, rnd, j)
                if order != ident(N):
                    assert not np.array_equal(op.fold(port, dt, ins, order),
                                              op.fold(port, dt, ins, ident(N))), (rnd, j)


@pytest.mark.parametrize("case", [c for c in FLOAT_CASES if c[0] > 8], ids=ss.case_id)
def test_dropped_second_release_word_changes_every_probed_tile(port, case):
    """Positions 8.. of the order reset to their identity values (PermSrcs16
    without the block's second word) change bytes in every probed tile,
    whenever the reset differs from the order (9 workers: unless worker 8
    came last); with 12 workers or more among them NaN-result probes."""
    N, dt, vpt = case
    hit = 0
    for rnd, j, ins, kind, order, want in rounds_of(port, case):
        reset = op.second_word_reset(order)
        if reset == order:
            assert N == 9
            continue
        hit += 1
        d = op.changed(dt, want, op.fold(port, dt, ins, reset))
        for name, (lo, hi) in probed_tiles(dt, vpt, j):
            assert d[lo:hi].any(), (rnd, j, name)
            if N >= 12:
                assert (d & (kind >= 0) & op.is_nan(dt, want))[lo:hi].any(), (rnd, j, name)
    assert hit >= 4


@FLOATS
def test_dropped_last_valid_slot_of_the_partial_tile_shows(port, case):
    """A partial tile whose last valid slot is not written keeps what the
    store held: the previous round's result (zeros after the init round).
    More than half of that slot's elements differ from the oracle's in every
    round (the probes sit at the same elements in every round and may give
    the same NaN; the background is the round's own)."""
    N, dt, vpt = case
    es = elem_size(dt)
    reg = ss.key_regions(dt, vpt, ss.RAGGED)["partial_tile"]
    last = max(s for s, k in enumerate(ss.slot_vecs(vpt)) if k)
    lo, hi = fs.slot(dt, reg, last)
    assert (hi - lo) // fs.vec_elems(dt) == ss.slot_vecs(vpt)[last]
    before = np.zeros(ss.key_elems(dt, vpt)[ss.RAGGED] * es, np.uint8)
    for rnd, j, ins, kind, order, want in rounds_of(port, case):
        if j != ss.RAGGED:
            continue
        d = op.changed(dt, want, before)[lo:hi]
        assert d.mean() > 0.5, rnd
        before = want
