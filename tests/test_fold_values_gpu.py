"""The fold operators of prophet_amd/csrc/bpsr_ops.h on the enumerated operand
tables of tests/fold_values.py (every fp16 / bf16 pattern against partners
built from it; the boundary cross products of f32 / f64; every int8 pair; the
int32 / int64 boundaries and carries), on every fold path, every comparison
on the raw bytes with no tolerance.

Reference mode is compared with oracle.oracle.PortReducer, fp32-accumulate
mode with tests/accum_model.py; tests/test_fold_values.py checks on the CPU
that those agree with the reference's own reducer on these inputs and that
every value class occurs often enough.  The other fold tests pin where an
element sits (tile, lane, head, tail, VPT, store policy); these pin which
values meet: subnormal inputs and results, the sign of a zero, exact ties and
their neighbours, the overflow boundary, the carry between the words of an
int64, a NaN against every class of partner in both orders.

Paths: sum_n on co-aligned operands (the vector fast path and the NaN
replay; the tables are NaN-dense on purpose) and with one source shifted by
an element (the whole table through fold_elements), sum in place, sum3, the
n-way chains (compile-time and generic source counts, the pointer table, the
chained launch of n = 33), sum_batched and a plan over ragged buckets, a block
queue in both shapes.  All at VPT 1 or whatever the launcher picks: the
operators do not depend on the tile, and test_fold_tiles_gpu.py covers it.
dst is prefilled with 0x5A, 0xEE guard bytes lie around dst and every source,
and no source may change (fold_run.Operands).
"""
import warnings

import numpy as np
import pytest

import accum_model as am
import fold_shapes as fs
import fold_values as fv
from fold_run import Operands, assert_elements
from oracle.oracle import PortReducer
from prophet_amd.dtypes import ALL_DTYPES, DType, elem_size

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MODE_REFERENCE, MODE_ACCUM_F32 = 0, 1

# (dtype, mode): reference mode for every dtype, fp32-accumulate for the 16-bit floats
PATHS = [(dt, MODE_REFERENCE) for dt in ALL_DTYPES] + [(dt, MODE_ACCUM_F32) for dt in fv.FLOATS_16]
ON_PATHS = pytest.mark.parametrize(
    "dt,mode", PATHS, ids=[f"{DType(d).name}{'-accum_f32' if m else ''}" for d, m in PATHS])
ON_DTYPES = pytest.mark.parametrize("dt", list(ALL_DTYPES), ids=lambda d: DType(d).name)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def red(dev):
    from prophet_amd.reducer import GpuReducer
    return GpuReducer(device=0)


def host(x: np.ndarray):
    """A pattern array as a host byte tensor (the tables are read-only; nothing
    writes through it)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return torch.from_numpy(fv.as_bytes(x))


def fold_want(dt, mode, srcs) -> np.ndarray:
    """The expected bytes of one left fold of pattern arrays."""
    by = [fv.as_bytes(s) for s in srcs]
    if mode == MODE_ACCUM_F32:
        return am.fold_bytes(by, len(by[0]), DType(dt) == DType.BFLOAT16)
    return fs.oracle_fold(dt, by, len(by[0]))


_WANT = {}      # (dtype, mode, n sources or a tag) -> expected bytes, shared, never modified


def table_want(dt, mode, n: int):
    """(sources, kinds, expected bytes) of the pair table (n = 2) or a chain."""
    if n == 2:
        a, b, kind = fv.pair_table(dt)
        srcs = [a, b]
    else:
        srcs, kind = fv.chain_sources(dt, n)
    key = (int(dt), mode, n)
    if key not in _WANT:
        _WANT[key] = fold_want(dt, mode, srcs)
    return srcs, kind, _WANT[key]


def run_sum_n(red, dev, dt, mode, srcs, src_offs=None):
    L = srcs[0].nbytes
    ops = Operands(dev, len(srcs), L, src_offs).load([host(s) for s in srcs])
    torch.cuda.synchronize()
    red.sum_n(ops.dst, ops.srcs, L, dt, mode=mode)
    torch.cuda.synchronize()
    return ops.result()


# ---------------------------------------------------------------- two sources ----

@ON_PATHS
@pytest.mark.parametrize("shifted", [False, True], ids=["coaligned", "source_shifted"])
def test_sum_n_pairs(red, dev, dt, mode, shifted):
    """Co-aligned: full and partial vector tiles, the fast path (fast /
    finish_fast: v_pk_add_f16, v_cvt_pk_bf16_f32, the packed narrowings of
    OpAcc16) and, for every vector that holds a NaN, the exact replay (accum /
    finish: f16x2_add_body, bf16_add and f32_to_bf16_rne, f64_add).  With
    source 1 one element further inside its 16-byte line there is no vector
    range and the whole table goes through fold_elements (accum_e:
    f16_add_elem, bf16_add, f32_add, f64_add, down)."""
    srcs, kind, want = table_want(dt, mode, 2)
    got = run_sum_n(red, dev, dt, mode, srcs, [0, elem_size(dt)] if shifted else None)
    assert_elements(dt, got, want, kind, "pairs")


@pytest.mark.parametrize("shifted", [False, True], ids=["coaligned", "source_shifted"])
def test_fp16_tail_length(red, dev, shifted):
    """The fp16 table at the length with n % 8 == 5: its last five rows, NaN
    against NaN, lie in the reference's scalar tail, where every NaN becomes
    0x7fff; the rows before them keep their payloads."""
    dt = DType.FLOAT16
    a, b, kind = fv.pair_table(dt)
    n = fv.fp16_tail_cut()
    srcs = [np.ascontiguousarray(a[:n]), np.ascontiguousarray(b[:n])]
    key = (int(dt), MODE_REFERENCE, "tail")
    if key not in _WANT:
        _WANT[key] = fold_want(dt, MODE_REFERENCE, srcs)
    want = _WANT[key]
    assert bool((want.view(np.uint16)[-5:] == 0x7FFF).all())
    got = run_sum_n(red, dev, dt, MODE_REFERENCE, srcs, [0, 2] if shifted else None)
    assert_elements(dt, got, want, kind[:n], "n % 8 == 5")


@ON_DTYPES
def test_sum_in_place(red, dev, dt):
    """byteps_reduce_sum: dst += src, dst the first operand."""
    (a, b), kind, want = table_want(dt, MODE_REFERENCE, 2)
    L = a.nbytes
    ops = Operands(dev, 2, L, inplace=True).load([host(a), host(b)])
    torch.cuda.synchronize()
    red.sum(ops.dst, ops.srcs[1], L, dt)
    torch.cuda.synchronize()
    assert_elements(dt, ops.result(), want, kind, "sum")


@ON_DTYPES
@pytest.mark.parametrize("swapped", [False, True], ids=["a_b", "b_a"])
def test_sum3(red, dev, dt, swapped):
    """byteps_reduce_sum3: dst = src1 + src2, in both operand orders, against
    the oracle's sum3 (fp16 keeps src2's NaN where both are NaN, as the
    compiled reference does; every other dtype src1's)."""
    a, b, kind = fv.pair_table(dt)
    s1, s2 = (b, a) if swapped else (a, b)
    L = a.nbytes
    key = (int(dt), "sum3", swapped)
    if key not in _WANT:
        want = np.full(L, 0x5A, np.uint8)
        assert PortReducer(nthreads=8).sum3(want, s1, s2, L, dt) == 0
        _WANT[key] = want
    ops = Operands(dev, 2, L).load([host(s1), host(s2)])
    torch.cuda.synchronize()
    red.sum3(ops.dst, ops.srcs[0], ops.srcs[1], L, dt)
    torch.cuda.synchronize()
    assert_elements(dt, ops.result(), _WANT[key], kind, "sum3")


# --------------------------------------------------------------------- chains ----

@ON_PATHS
@pytest.mark.parametrize("n", [3, 9, 17, 33])
def test_sum_n_chain(red, dev, dt, mode, n):
    """The hand-written triples and the pair table under rolled further
    sources: n = 3 and 9 on the generic kernel (pointers in SGPRs up to 8
    sources, the pointer table above), 17 the same with two load groups, 33
    the chained launch (32 sources fold, and narrow in fp32-accumulate mode,
    then [result] + 1 in place)."""
    srcs, kind, want = table_want(dt, mode, n)
    got = run_sum_n(red, dev, dt, mode, srcs)
    assert_elements(dt, got, want, kind, f"n={n}")


# ------------------------------------------------------------ ragged buckets ----

def ragged_buckets(dt):
    """The pair table cut into buckets: (first element, elements, byte offsets
    of dst and the two sources).  One bucket is co-aligned one element inside
    its 16-byte line (a head through fold_elements, then vector tiles), one
    has a single source shifted by an element (element work only), one is
    empty; the last takes what is left."""
    es = elem_size(dt)
    N = len(fv.pair_table(dt)[0])
    sizes = [1, 9, max(N // 50, 11), 0, N // 3 + 5, N // 7 + 3]
    offs = [None, None, [es, es, es], None, None, [0, 0, es]]
    sizes.append(N - sum(sizes))
    offs.append(None)
    assert sizes[-1] > 0
    out, at = [], 0
    for ne, o in zip(sizes, offs):
        out.append((at, ne, o or [0, 0, 0]))
        at += ne
    return out


def bucket_hosts(dt, mode, swapped: bool):
    """Per bucket: (host sources, kinds, expected bytes).  Every bucket is a
    fold of its own (the fp16 tail is the last n % 8 elements of the bucket)."""
    key = (int(dt), mode, "buckets", swapped)
    if key not in _WANT:
        a, b, kind = fv.pair_table(dt)
        if swapped:
            a, b = b, a
        rows = []
        for at, ne, _ in ragged_buckets(dt):
            srcs = [np.ascontiguousarray(x[at:at + ne]) for x in (a, b)]
            want = fold_want(dt, mode, srcs) if ne else np.zeros(0, np.uint8)
            rows.append(([host(s) for s in srcs], kind[at:at + ne], want))
        _WANT[key] = rows
    return _WANT[key]


def bucket_operands(dev, dt):
    es = elem_size(dt)
    return [Operands(dev, 2, ne * es, o[1:], o[0]) for _, ne, o in ragged_buckets(dt)]


def load_and_check(ops, rows, dt, what):
    def check():
        for i, (o, (_, kind, want)) in enumerate(zip(ops, rows)):
            assert_elements(dt, o.result(), want, kind, f"{what} bucket {i}")
    for o, (ins, _, _) in zip(ops, rows):
        o.load(ins)
    torch.cuda.synchronize()
    return check


@ON_PATHS
@pytest.mark.parametrize("plan", [False, True], ids=["one_off", "plan"])
def test_batched_ragged_buckets(red, dev, dt, mode, plan):
    """batched_kernel (run_record) over the table cut into ragged buckets, as
    a one-off launch and as a plan launched a second time with the operands
    swapped at the same addresses (b + a: every NaN row in the other order)."""
    ops = bucket_operands(dev, dt)
    buckets = [o.bucket for o in ops]
    check = load_and_check(ops, bucket_hosts(dt, mode, False), dt, "a + b")
    if not plan:
        red.sum_batched(buckets, dt, mode=mode)
        torch.cuda.synchronize()
        check()
        return
    p = red.make_plan(buckets, dt, mode=mode)
    p.launch()
    torch.cuda.synchronize()
    check()
    check = load_and_check(ops, bucket_hosts(dt, mode, True), dt, "b + a")
    p.launch()
    torch.cuda.synchronize()
    check()
    p.close()


@ON_PATHS
@pytest.mark.parametrize("shape", [0, 1], ids=["dispatch", "persistent"])
def test_blockq_release_all_two_iterations(red, dev, dt, mode, shape):
    """blockq_gate_kernel (wg_per_cu 0, one record per workgroup) and
    blockq_kernel (the persistent sweep): the ragged buckets in four blocks,
    one of them empty, everything released up front; the second iteration has
    the operands swapped."""
    ops = bucket_operands(dev, dt)
    b = [o.bucket for o in ops]
    q = red.make_blockq([b[0:2], [], b[2:5], b[5:]], dt, mode)
    q.config(wg_per_cu=shape)
    for it in range(2):
        check = load_and_check(ops, bucket_hosts(dt, mode, it == 1), dt, f"iteration {it}")
        q.release(-1)
        q.launch()
        q.status()
        torch.cuda.synchronize()
        check()
    q.close()
