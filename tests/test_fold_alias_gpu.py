"""Aliased operands on every fold entry, at the tile sizes real folds run.

The parity claim is "drop-in for CpuReducer", whose loops are element-wise:
any exact alias between operands is legal there.  The kernels keep that
because each lane stores slot j only after its loads and its exact replay of
slot j; a kernel that stored the fast result first and patched the NaN
vectors afterwards, or an element path that stored between its load groups,
would be right for a dst of its own and wrong here.  So every form the entry
points accept runs on fold_shapes' V2 / V4 / SMALL shapes (2,047 full tiles, a
partial tile, a head, a tail; order_probe's NaN / inf probes, so the replay
runs in every probed tile), every comparison on the raw bytes against
oracle.oracle.PortReducer called on the same operand list — tests/
test_fold_alias.py pins on the CPU that the port with aliased arrays is the
compiled reference with aliased arrays:

  a. byteps_reduce_sum3: dst is src1, dst is src2, src1 is src2, all three
     one buffer (fp16 folds src2 first, so sum3(x, x, y) has dst at srcs[1]);
  b. byteps_reduce_sum(dst, dst);
  c. duplicate read-only sources in sum_n (also with dst at srcs[0]), in both
     modes for the 16-bit types, and in two buckets of a batched launch, a
     plan and a block queue;
  d. dst at srcs[k], k > 0 (fold_any_alias), through the shard ABI's
     in-process groups: reduce_scatter in place at world 3 (k = rank) with the
     in-place allgather, reduce_root in place at world 8 with root 5 and the
     broadcast, and scatter_reduce of landed pushes into one of them with k
     in the second load group (k = 8 of 9, k = 9 of 12);
  e. what is refused stays refused before anything is written: EARGS, and
     every operand's bytes and guard bytes as they were.

0xEE guard bytes lie around every distinct buffer and no buffer but dst's
may change (fold_run.Operands, fold_run.Guarded).  tests/test_fold_shapes.py
checks on the CPU that every case gets the tile size, kernel and policy its id
names and that the aliased source holds NaNs where a peer holds one too.
"""
import threading

import numpy as np
import pytest

import accum_model as am
import fold_shapes as fs
from fold_run import FILL, Guarded, Operands, assert_elements
from oracle.oracle import PortReducer
from prophet_amd.dtypes import DType, elem_size
from test_fold_tiles_gpu import check_batched, check_blockq

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MODE_REFERENCE, MODE_ACCUM_F32 = 0, 1
_F16, _F32, _BF16 = DType.FLOAT16, DType.FLOAT32, DType.BFLOAT16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def red(dev):
    from prophet_amd.reducer import GpuReducer
    return GpuReducer(device=0)


def mode_ids(cases):
    """Every case in reference mode, the 16-bit floats also in fp32-accumulate."""
    out = [(c, MODE_REFERENCE) for c in cases]
    out += [(c, MODE_ACCUM_F32) for c in cases if c[0] in (_F16, _BF16)]
    return pytest.mark.parametrize(
        "case,mode", out, ids=[fs.alias_id(c) + ("-accum_f32" if m else "") for c, m in out])


_WANT = {}      # expected bytes, shared, never modified


def want_of(case, mode):
    """(sources, kinds, expected bytes) of a case of fold_shapes.ALIAS."""
    ins, kind, want, _ = fs.alias_case(case)
    if mode == MODE_ACCUM_F32:
        key = (case, mode)
        if key not in _WANT:
            _WANT[key] = am.fold_bytes(ins, len(want), case[0] == _BF16)
        want = _WANT[key]
    return ins, kind, want


# --------------------------------------------------------------- a. sum3 ----

SUM3_FORMS = ("dst_is_src1", "dst_is_src2", "src1_is_src2", "all_one")


def sum3_want(case, form, x, y):
    """The port's sum3 of a case's two inputs, the host arrays aliased as
    `form` says."""
    dt, key = case[0], (case, form)
    if key not in _WANT:
        port, L = PortReducer(nthreads=8), len(x)
        a, b = x.copy(), y.copy()
        if form == "dst_is_src1":
            assert port.sum3(a, a, b, L, dt) == 0
            out = a
        elif form == "dst_is_src2":
            assert port.sum3(b, a, b, L, dt) == 0
            out = b
        elif form == "src1_is_src2":
            out = np.full(L, FILL, np.uint8)
            assert port.sum3(out, a, a, L, dt) == 0
        else:
            assert port.sum3(a, a, a, L, dt) == 0
            out = a
        _WANT[key] = out
    return _WANT[key]


def sum3_operands(dev, form, L, off):
    """(operands, dst, src1, src2) of a form: two sources x, y in buffers of
    their own; dst as the form says."""
    alias = {"dst_is_src1": 0, "dst_is_src2": 1, "src1_is_src2": None, "all_one": 0}[form]
    ops = Operands(dev, 2, L, [off, off], 16 + off, alias=alias)
    x, y = ops.srcs
    return ops, {"dst_is_src1": (x, x, y), "dst_is_src2": (y, x, y),
                 "src1_is_src2": (ops.dst, x, x), "all_one": (x, x, x)}[form]


@pytest.mark.parametrize("form", SUM3_FORMS)
@pytest.mark.parametrize("case", fs.SUM3_CASES, ids=fs.case_id)
def test_sum3_aliased(red, dev, case, form):
    """fold_kernel<NS 2> at 16 KiB tiles (n <= 4: tuning_for_n), SMALL, and
    SMALL 8 bytes into the 16-byte line (a head through fold_elements).  fp16
    launches [src2, src1]: dst_is_src1 has dst at srcs[1] there, dst_is_src2
    at srcs[0]; every other dtype the other way round."""
    dt, _, shape = case[:3]
    off = case[3] if len(case) > 3 else 0
    ins, kind, want, _ = fs.fold_case(dt, 2, shape, off)
    L = len(want)
    ops, (d, s1, s2) = sum3_operands(dev, form, L, off)
    ops.load(ins)
    torch.cuda.synchronize()
    red.sum3(d, s1, s2, L, dt)
    torch.cuda.synchronize()
    assert_elements(dt, ops.result(), sum3_want(case, form, ins[0], ins[1]), kind,
                    f"sum3 {form} {fs.case_id(case)}")


@pytest.mark.parametrize("dt", [_F16, _F32], ids=lambda d: DType(d).name)
def test_sum3_torch_op_dst_is_src1(dev, dt):
    """torch.ops.bpsr.sum3_(x, x, y)."""
    from prophet_amd import torch_ops  # noqa: F401  (registers torch.ops.bpsr.*)
    ins, kind, want, _ = fs.fold_case(dt, 2, "V4")
    tdt = {_F16: torch.float16, _F32: torch.float32}[dt]
    x, y = (torch.from_numpy(v).to(dev).view(tdt) for v in ins)
    torch.ops.bpsr.sum3_(x, x, y)
    torch.cuda.synchronize()
    assert_elements(dt, x.view(torch.uint8).cpu().numpy(),
                    sum3_want((dt, 2, "V4"), "dst_is_src1", ins[0], ins[1]), kind,
                    "sum3_(x, x, y)")
    assert np.array_equal(y.view(torch.uint8).cpu().numpy(), ins[1])


# ------------------------------------------------------- b. sum(dst, dst) ----

@pytest.mark.parametrize("case", fs.DOUBLING, ids=fs.case_id)
def test_sum_dst_dst(red, dev, case):
    """byteps_reduce_sum(x, x): both sources of the launch are dst."""
    dt, _, shape = case
    ins, kind, _, _ = fs.fold_case(dt, 2, shape)
    x, L = ins[0], len(ins[0])
    want = x.copy()
    assert PortReducer(nthreads=8).sum(want, want, L, dt) == 0
    ops = Operands(dev, 1, L, alias=0).load([x])
    torch.cuda.synchronize()
    red.sum(ops.dst, ops.dst, L, dt)
    torch.cuda.synchronize()
    assert_elements(dt, ops.result(), want, kind, "sum(x, x)")


# ------------------------------------------------- c. duplicate sources ----

@mode_ids(fs.ALIAS_DUP)
def test_sum_n_duplicate_sources(red, dev, case, mode):
    """sum_n(dst, [a, a, b, ...]) and sum_n(a, [a, b, b, ...]); above 8
    sources a second pair has its later member in the second load group.
    n = 3 and 9 on the generic kernel, 8 and 16 on the NS kernels."""
    dt, n, _, alias, same = case
    ins, kind, want = want_of(case, mode)
    L = len(want)
    ops = Operands(dev, n, L, alias=alias, same=same).load(ins)
    torch.cuda.synchronize()
    red.sum_n(ops.dst, ops.srcs, L, dt, mode=mode)
    torch.cuda.synchronize()
    assert_elements(dt, ops.result(), want, kind, fs.alias_id(case))


@pytest.mark.parametrize("dt", [_F32, _F16], ids=lambda d: DType(d).name)
@pytest.mark.parametrize("plan", [False, True], ids=["one_off", "plan"])
def test_batched_duplicate_sources(red, dev, dt, plan):
    """The ragged table at VPT 2 with a duplicated source in its 8-source
    bucket (register path) and its 9-source bucket (pointer array, across the
    load groups), as a one-off launch and as a plan launched twice."""
    check_batched(red, dev, dt, 2, plan, dups=fs.TABLE_DUPS)


@pytest.mark.parametrize("dt", [_F32, _F16], ids=lambda d: DType(d).name)
@pytest.mark.parametrize("shape", [0, 1], ids=["dispatch", "persistent"])
def test_blockq_duplicate_sources(red, dev, monkeypatch, dt, shape):
    """The same two buckets of the block queue's table, both consumers."""
    monkeypatch.setenv("BPSR_BQ_VPT", "2")
    check_blockq(red, dev, dt, shape, 2, 2, dups=fs.TABLE_DUPS)


# ------------------------------------ d. dst at srcs[k], k > 0: shard ABI ----

def run_ranks(world, fn):
    """fn(rank, stream) on one host thread per rank; the first failure."""
    errs, out = [None] * world, [None] * world

    def body(r):
        try:
            s = torch.cuda.Stream(device=0)
            with torch.cuda.stream(s):
                out[r] = fn(r, s)
            s.synchronize()
        except BaseException as e:   # noqa: BLE001 - re-raised below
            errs[r] = e
    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=120)
        assert not t.is_alive(), "shard group thread hung"
    for e in errs:
        if e is not None:
            raise e
    return out


def fold_want(dt, mode, ins, L):
    if mode == MODE_ACCUM_F32:
        return am.fold_bytes(ins, L, dt == _BF16)
    return fs.oracle_fold(dt, ins, L)


SCATTER = [(_F32, MODE_REFERENCE), (_F16, MODE_REFERENCE), (_F16, MODE_ACCUM_F32)]


@pytest.mark.parametrize("dt,mode", SCATTER,
                         ids=[DType(d).name + ("-accum_f32" if m else "") for d, m in SCATTER])
def test_reduce_scatter_in_place_then_allgather(dev, dt, mode):
    """PostNcclCalls with tensor == output at world 3: rank r folds into its
    slice of its own vector (dst = p + lo: srcs[r] of the generic kernel),
    every slice 2,047 full tiles of VPT 4, a partial one, a head and a tail;
    ranks 1 and 2 own slices that begin inside a 16-byte line.  Then the
    all-gather in place.  Every rank's vector must be each owner's slice
    folded in rank order; no receive slot's guard bytes may change."""
    from prophet_amd.shard import ShardComm, owner_ranges
    world, es = 3, elem_size(dt)
    E, full, kind, offs = fs.scatter_vectors(dt, world, "V4", 77)
    ranges = owner_ranges(E, world)
    want = np.concatenate([fold_want(dt, mode, [v[lo * es:hi * es] for v in full], (hi - lo) * es)
                           for lo, hi in ranges])
    vec = [Guarded(dev, E * es).load(full[r]) for r in range(world)]
    slots = [[Guarded(dev, (ranges[r][1] - ranges[r][0]) * es, offs[r]) if q != r else None
              for q in range(world)] for r in range(world)]
    torch.cuda.synchronize()
    comms = ShardComm.local_group([0] * world)

    def rank(r, s):
        lo, _ = ranges[r]
        p = vec[r].ptr
        comms[r].reduce_scatter(p, [g.ptr if g else 0 for g in slots[r]], p + lo * es,
                                elems=E, dtype=dt, mode=mode, stream=s)
        comms[r].allgather(p + lo * es, p, elems=E, dtype=dt, stream=s)
    run_ranks(world, rank)
    torch.cuda.synchronize()
    for r in range(world):
        assert_elements(dt, vec[r].bytes(f"rank {r}"), want, kind, f"rank {r}")
        lo, hi = ranges[r]
        for q, g in enumerate(slots[r]):
            if g is not None:       # a read-only source: still rank q's slice
                assert np.array_equal(g.bytes(f"rank {r} slot {q}"), full[q][lo * es:hi * es])
    for c in comms:
        c.close()


@pytest.mark.parametrize("case", fs.ALIAS_ROOT, ids=fs.alias_id)
def test_reduce_root_in_place_then_broadcast(dev, case):
    """BYTEPS_REDUCE_ROOTS at world 8, root 5: the root folds into its own
    vector (dst = local: srcs[5] of the NS = 8 kernel at VPT 2), then the
    broadcast; every rank must hold the 8-way fold in rank order."""
    from prophet_amd.shard import ShardComm
    dt, world, _, root, _ = case
    ins, kind, want, _ = fs.alias_case(case)
    L = len(want)
    E = L // elem_size(dt)
    vec = [Guarded(dev, L).load(ins[r]) for r in range(world)]
    slots = [Guarded(dev, L) if q != root else None for q in range(world)]
    torch.cuda.synchronize()
    comms = ShardComm.local_group([0] * world)

    def rank(r, s):
        p = vec[r].ptr
        recv = [g.ptr if g else 0 for g in slots] if r == root else None
        comms[r].reduce_root(root, p, recv, p, elems=E, dtype=dt, stream=s)
        comms[r].broadcast(root, p, elems=E, dtype=dt, stream=s)
    run_ranks(world, rank)
    torch.cuda.synchronize()
    for r in range(world):
        assert_elements(dt, vec[r].bytes(f"rank {r}"), want, kind, f"rank {r} (root {root})")
    for q, g in enumerate(slots):
        if g is not None:
            assert np.array_equal(g.bytes(f"slot {q}"), ins[q])
    for c in comms:
        c.close()


@mode_ids(fs.ALIAS_LANDED)
def test_scatter_reduce_into_a_late_push(dev, case, mode):
    """Landed pushes folded into one of them on a group of one rank: dst is
    srcs[8] of 9 (V2: the tiles' second load group and fold_elements' second
    group of 8) and srcs[9] of 12 (SMALL)."""
    from prophet_amd.shard import ShardComm
    dt, n, _, alias, same = case
    ins, kind, want = want_of(case, mode)
    L = len(want)
    ops = Operands(dev, n, L, alias=alias, same=same).load(ins)
    torch.cuda.synchronize()
    comm = ShardComm.local_group([0])[0]
    comm.scatter_reduce(0, ops.srcs, None, ops.dst, L // elem_size(dt), dt, mode=mode)
    torch.cuda.synchronize()
    assert_elements(dt, ops.result(), want, kind, fs.alias_id(case))
    comm.close()


# ------------------------------------------------ e. refused, nothing written ----

def refused(call, ops, what):
    from prophet_amd.reducer import EARGS, ReduceError
    with pytest.raises(ReduceError) as e:
        call()
    assert e.value.code == EARGS, what
    torch.cuda.synchronize()
    for o in ops:
        o.untouched(what)


def small_operands(dev, n, **kw):
    dt = _F32
    ins, _, want, _ = fs.fold_case(dt, n, "SMALL")
    return Operands(dev, n, len(want), **kw).load(fs.share(ins, kw.get("same", ()))), len(want)


def test_refused_sum_n_dst_at_a_later_source(red, dev):
    ops, L = small_operands(dev, 3, alias=1)
    torch.cuda.synchronize()
    refused(lambda: red.sum_n(ops.dst, ops.srcs, L, _F32), [ops], "sum_n, dst is srcs[1]")
    both, L = small_operands(dev, 3, alias=0, same=((0, 2),))
    torch.cuda.synchronize()
    refused(lambda: red.sum_n(both.dst, both.srcs, L, _F32), [both], "sum_n, dst is srcs[0] and [2]")


def test_refused_partial_overlaps(red, dev):
    """dst 16 bytes into a source, on sum, sum3, sum_n and a batched bucket,
    a plan and a block queue; the calls take 64 bytes fewer than the buffers
    hold, so every range named lies inside them."""
    ops, L = small_operands(dev, 2)
    torch.cuda.synchronize()
    x, y = ops.srcs
    n = L - 64
    refused(lambda: red.sum(x + 16, x, n, _F32), [ops], "sum")
    refused(lambda: red.sum3(x + 16, x, y, n, _F32), [ops], "sum3, dst into src1")
    refused(lambda: red.sum3(y + 16, x, y, n, _F32), [ops], "sum3, dst into src2")
    refused(lambda: red.sum_n(y + 16, [x, y], n, _F32), [ops], "sum_n")
    bucket = [(y + 16, [x, y], n)]
    refused(lambda: red.sum_batched(bucket, _F32), [ops], "sum_batched")
    refused(lambda: red.make_plan(bucket, _F32), [ops], "plan")
    refused(lambda: red.make_blockq([bucket], _F32), [ops], "block queue")


def test_refused_bucket_dst_at_srcs_1(red, dev):
    ops, L = small_operands(dev, 3, alias=1)
    good, _ = small_operands(dev, 3)
    torch.cuda.synchronize()
    table = [good.bucket, ops.bucket]
    refused(lambda: red.sum_batched(table, _F32), [ops, good], "sum_batched")
    refused(lambda: red.make_plan(table, _F32), [ops, good], "plan")
    refused(lambda: red.make_blockq([[good.bucket], [ops.bucket]], _F32), [ops, good],
            "block queue")


def test_refused_reduce_scatter_slot_is_dst(dev):
    """In place at world 2 with the peer's receive slot at dst as well: dst
    would alias two sources.  Both ranks are refused before a receive writes
    into the slot, so each rank's vector is as it was."""
    from prophet_amd.reducer import EARGS, ReduceError
    from prophet_amd.shard import ShardComm, owner_ranges
    world, E = 2, 2 * 4099
    ranges = owner_ranges(E, world)
    data = [fs.probe_inputs(_F32, E, 1, 50 + r, {})[0][0] for r in range(world)]
    vec = [Guarded(dev, E * 4).load(data[r]) for r in range(world)]
    torch.cuda.synchronize()
    comms = ShardComm.local_group([0] * world)

    def rank(r, s):
        dst = vec[r].ptr + ranges[r][0] * 4
        with pytest.raises(ReduceError) as e:
            comms[r].reduce_scatter(vec[r].ptr, [dst, dst], dst, elems=E, dtype=_F32, stream=s)
        return e.value.code, str(e.value)
    for code, msg in run_ranks(world, rank):
        assert code == EARGS and "two sources" in msg, msg
    torch.cuda.synchronize()
    for r in range(world):
        assert np.array_equal(vec[r].bytes(f"rank {r}"), data[r]), f"rank {r}'s vector changed"
    for c in comms:
        c.close()


def test_refused_dst_at_a_later_source_of_33(dev):
    """fold_any_alias folds in one launch: dst at srcs[k > 0] of more than 32
    sources is refused (scatter_reduce of 33 landed pushes into pushes[5])."""
    from prophet_amd.shard import ShardComm
    ins, _, want, _ = fs.fold_case(_F32, 3, "SMALL")
    L = len(want)
    ops = Operands(dev, 33, L, alias=5).load([ins[k % 3] for k in range(33)])
    torch.cuda.synchronize()
    comm = ShardComm.local_group([0])[0]
    refused(lambda: comm.scatter_reduce(0, ops.srcs, None, ops.dst, L // 4, _F32), [ops],
            "33 pushes, dst is pushes[5]")
    comm.close()
