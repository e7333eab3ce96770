"""GPU parity of BYTEPS_REDUCE_MODE_ACCUM_F32 (fp16 / bf16 folded in fp32,
OpAcc16 in prophet_amd/csrc/bpsr_ops.h) on every fold path, bit for bit
against the numpy model of tests/accum_model.py (itself checked on the CPU by
tests/test_accum_model.py).

Every comparison is on the raw bytes, with no tolerance.  Inputs are the
model's order-sensitive ``cancel`` class (a wrong summation order, a narrowing
after every add or a truncating narrowing changes well over 1 % of the
elements, asserted by test_accum_model.py) and synth's ``bits`` / ``special`` classes (subnormals,
overflow to Inf, NaN / Inf inputs: the exact replay of vectors whose fast
result holds a NaN).

Geometry: a tile is 256 threads x VPT 16-byte vectors.  At the small sizes
fold_vpt (bpsr_internal.h) picks VPT 1, so a tile holds 2,048 16-bit elements;
SMALL is 3 full tiles (fold_tile_full_buf), a guarded partial tile
(fold_tile_body) and a ragged element tail (fold_elements).
"""
import numpy as np
import pytest

import accum_model as am
import fold_run
from prophet_amd.dtypes import DType
from test_blockq_gpu import MIXED, Table
from test_parity_gpu import ptr, to_dev

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MODE_REFERENCE, MODE_ACCUM_F32 = 0, 1
SMALL = 3 * 2048 + 805
DTYPES = pytest.mark.parametrize("dt", [DType.FLOAT16, DType.BFLOAT16],
                                 ids=lambda d: DType(d).name)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def red(dev):
    from prophet_amd.reducer import GpuReducer
    return GpuReducer(device=0)


def is_bf(dt) -> bool:
    return DType(dt) == DType.BFLOAT16


def assert_same(got: np.ndarray, want: np.ndarray, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} bytes differ, first at byte {i} "
                             f"(element {i // 2}): got {int(got[i]):#04x}, want {int(want[i]):#04x}")


def run_sum_n(red, dev, dt, ins, L, src_offs=None, dst_off=16, inplace=False,
              mode=MODE_ACCUM_F32):
    """sum_n of host byte arrays `ins` placed at byte offsets `src_offs` of
    0xEE-filled buffers, into a 0x5A-prefilled dst at `dst_off` (or into
    srcs[0]).  Checks the guard bytes around dst and every source and that no
    source other than an aliased srcs[0] changed (fold_run.Operands); returns
    dst's L bytes."""
    return fold_run.run_sum_n(red, dev, dt, ins, L, src_offs, dst_off, inplace, mode)


# ------------------------------------------------------------ sum_n, small ----

@DTYPES
@pytest.mark.parametrize("cls", ["cancel", "bits", "special"])
@pytest.mark.parametrize("n", [2, 3, 8, 9, 16, 32, 40])
def test_sum_n_small_shape(red, dev, dt, n, cls):
    """fold_kernel at VPT 1: NS = 2, 8, 16 (compile-time source counts) and the
    generic NS = 0 (n = 3, 9, 32); n = 40 is the chain of byteps_reduce_sum_n
    (32 sources fold and narrow, then [result] + 8, generic kernel, dst aliasing
    srcs[0]).  3 full tiles, the guarded partial tile, 5 tail elements through
    fold_elements (init_e / accum_e / finish_e).  `special` and, through
    inf + -inf, `bits` send vectors to the exact NaN replay
    (fold_vector_exact: init / accum / finish); `cancel` pins the order and
    the single RNE narrowing of init_fast / fast / finish_fast."""
    ins = am.inputs(dt, SMALL, n, cls, 11)
    got = run_sum_n(red, dev, dt, ins, 2 * SMALL)
    assert_same(got, am.fold_bytes(ins, 2 * SMALL, is_bf(dt)), f"n={n} {cls}")


@DTYPES
def test_sum_n_one_source_is_a_copy(red, dev, dt):
    """n = 1 goes to the copy kernel: signalling NaNs stay as they are."""
    ins = am.inputs(dt, SMALL, 1, "special", 12)
    emask, quiet = (0x7F80, 0x0040) if is_bf(dt) else (0x7C00, 0x0200)
    h = ins[0].view(np.uint16)
    snan = ((h & emask) == emask) & ((h & (emask ^ 0x7FFF)) != 0) & ((h & quiet) == 0)
    assert snan.any()                       # the inputs do hold signalling NaNs
    got = run_sum_n(red, dev, dt, ins, 2 * SMALL)
    assert_same(got, ins[0], "n=1")
    assert_same(got, am.fold_bytes(ins, 2 * SMALL, is_bf(dt)), "n=1 model")


@DTYPES
@pytest.mark.parametrize("cls", ["cancel", "special"])
@pytest.mark.parametrize("n", [8, 9])
@pytest.mark.parametrize("off", [2, 6, 14])
def test_sum_n_coaligned_byte_offsets(red, dev, dt, off, n, cls):
    """Every operand at the same byte offset inside its 16-byte line: an
    unaligned head of 7, 5 or 1 elements and a tail, both through
    fold_elements, around vector tiles (NS = 8 and generic)."""
    ins = am.inputs(dt, SMALL, n, cls, 13 + off)
    got = run_sum_n(red, dev, dt, ins, 2 * SMALL, src_offs=[off] * n, dst_off=16 + off)
    assert_same(got, am.fold_bytes(ins, 2 * SMALL, is_bf(dt)), f"off={off} n={n} {cls}")


@DTYPES
@pytest.mark.parametrize("n", [4, 12])
def test_sum_n_not_coaligned_operands(red, dev, dt, n):
    """Operands at different offsets, one not even element-aligned (the
    offsets of test_parity_gpu.test_not_coaligned_and_unaligned, repeated for
    n = 12): no vector range, the whole bucket goes through fold_elements with
    byte-wise loads and stores — the element path's exact fold, 8 sources per
    load group (n = 12: two groups), NaN / Inf inputs."""
    ne = 1007
    ins = am.inputs(dt, ne, n, "special", 14)
    offs = ([0, 2, 6, 1] * 3)[:n]
    got = run_sum_n(red, dev, dt, ins, 2 * ne, src_offs=offs, dst_off=5)
    assert_same(got, am.fold_bytes(ins, 2 * ne, is_bf(dt)), f"n={n}")


@DTYPES
@pytest.mark.parametrize("cls", ["cancel", "special"])
@pytest.mark.parametrize("n", [2, 8, 16, 40])
def test_sum_n_in_place(red, dev, dt, n, cls):
    """dst is srcs[0] (the zero-copy accumulator): every element is read
    before the same thread writes it, in the fast path and in the NaN replay,
    which re-reads srcs[0] from memory; n = 40 chains in place."""
    ins = am.inputs(dt, SMALL, n, cls, 15)
    got = run_sum_n(red, dev, dt, ins, 2 * SMALL, inplace=True)
    assert_same(got, am.fold_bytes(ins, 2 * SMALL, is_bf(dt)), f"in place n={n} {cls}")


@DTYPES
@pytest.mark.parametrize("n", [3, 8, 40])
def test_sum_n_odd_length(red, dev, dt, n):
    """len = 2 * n_elems + 1: the trailing byte of dst is srcs[0]'s, written by
    the first launch (fold_elements, copy_trailing); the chain's further
    launches (n = 40) fold in place and leave it."""
    ins = [np.concatenate([x, np.array([0x31 + k], np.uint8)])
           for k, x in enumerate(am.inputs(dt, SMALL, n, "special", 16))]
    L = 2 * SMALL + 1
    got = run_sum_n(red, dev, dt, ins, L)
    assert got[-1] == ins[0][-1] == 0x31
    assert_same(got, am.fold_bytes(ins, L, is_bf(dt)), f"odd n={n}")


# ------------------------------------------------ sum_n, the real tile sizes ----

@DTYPES
@pytest.mark.parametrize("n,nbytes,branch", [
    (3, (20 << 20) + 6, "VPT 2, generic NS"),
    (3, (36 << 20) + 6, "VPT 4, generic NS"),
    (8, (16 << 20) + 6, "VPT 2, NS = 8"),
], ids=["n3_20MiB_vpt2", "n3_36MiB_vpt4", "n8_16MiB_vpt2_ns8"])
def test_sum_n_real_tile_sizes(red, dev, dt, n, nbytes, branch):
    """The tile sizes of real launches (fold_vpt, tuning_for_n, launch_fold_op;
    kMinTiles = 2048, a tile is 4 KiB x VPT per operand):
      n = 3 starts at VPT 4 (tuning_for_n, n <= 4).  20 MiB is 1280 tiles of
        16 KiB, fewer than kMinTiles, so fold_vpt halves to VPT 2 (2560 tiles);
        36 MiB is 2304 tiles of 16 KiB and keeps VPT 4.
      n = 8 starts at VPT 2; 16 MiB is exactly 2048 tiles of 8 KiB, so VPT 2
        stays (and 1024 tiles of 16 KiB do not reach the mid-size VPT 4 rule),
        with the NS = 8 kernel.
    All are below 64 MiB per source: write-through stores, no half-tile band.
    The 6 extra bytes are 3 tail elements for fold_elements."""
    ne = nbytes // 2
    ins = am.inputs(dt, ne, n, "cancel", 17)
    srcs = [torch.from_numpy(x).to(dev) for x in ins]
    dbuf, _ = to_dev(np.full(nbytes, 0x5A, np.uint8), dev, offset=16)
    red.sum_n(ptr(dbuf, 16), srcs, nbytes, dt, mode=MODE_ACCUM_F32)
    torch.cuda.synchronize()
    whole = dbuf.cpu().numpy()
    assert bool((whole[:16] == 0xEE).all()) and bool((whole[16 + nbytes:] == 0xEE).all())
    assert_same(whole[16:16 + nbytes], am.fold_bytes(ins, nbytes, is_bf(dt)), branch)


# -------------------------------------------------- sum_batched and make_plan ----

# the table of test_parity_gpu.test_batched_ragged_mixed_table (element size 2)
# plus two `cancel` buckets: (n_elems, n_sources, offsets of dst + sources, class)
BATCH_SPEC = [
    (100_000, 8, None, "special"), (4099, 9, None, "normal"), (1, 1, None, "normal"),
    (70_001, 32, None, "bits"), (0, 8, None, "normal"), (3 * 1024 + 5, 2, [4, 4, 4], "normal"),
    (50_000, 3, [0, 2, 4, 1], "normal"), (257, 12, None, "special"),
    (300_000, 5, [2, 6, 10, 14, 2, 6], "normal"), (9, 8, None, "bits"),
    (SMALL, 8, None, "cancel"), (SMALL, 12, None, "cancel"),
    # one source is a byte copy in a table too: signalling NaNs stay as they are,
    # in vector tiles (the NaN replay), element tails and the element-only path
    (4099, 1, None, "special"), (300, 1, [0, 2], "special"),
]


def _batch_inputs(dt, seed):
    """Host inputs of every bucket and the model's expected bytes."""
    all_ins, wants = [], []
    for i, (ne, n, _, cls) in enumerate(BATCH_SPEC):
        ins = am.inputs(dt, ne, n, cls, seed + i)
        if i == 3:      # trailing bytes: one more element and a last odd byte
            ins = [np.concatenate([x, np.array([k, 7, 9], np.uint8)]) for k, x in enumerate(ins)]
        L = len(ins[0])
        all_ins.append(ins)
        wants.append(am.fold_bytes(ins, L, is_bf(dt)))
    return all_ins, wants


@DTYPES
@pytest.mark.parametrize("plan", [False, True], ids=["one_off", "plan"])
def test_batched_ragged_mixed_table(red, dev, dt, plan):
    """batched_kernel (run_record) with mode = ACCUM_F32 over one table mixing
    every tile kind: source counts 1..32 — the register path (n <= 8,
    NS = -8) and the N > 8 table path that reads the record's pointer array
    from memory (n = 9, 12, 32; `cancel` at 8 and 12) — full and partial vector
    tiles, co-aligned offsets (head + tail element tiles), operands that are
    not co-aligned (element tiles only, several parts), NaN / Inf inputs (the
    exact replay through the records' advanced pointers), trailing bytes, an
    empty bucket.  A plan is launched a second time on refilled sources."""
    all_ins, wants = _batch_inputs(dt, 300)
    buckets, views = [], []
    for (ne, n, offs, _), ins in zip(BATCH_SPEC, all_ins):
        L = len(ins[0])
        offs = offs or [0] * (n + 1)
        offs = (offs + [offs[-1]] * (n + 1))[:n + 1]
        bufs = [to_dev(x, dev, offset=o)[0] for x, o in zip(ins, offs[1:])]
        dbuf, _ = to_dev(np.full(L, 0x5A, np.uint8), dev, offset=offs[0])
        buckets.append((ptr(dbuf, offs[0]), [ptr(b, o) for b, o in zip(bufs, offs[1:])], L))
        views.append((dbuf, offs, L, bufs))

    def check(wants, what):
        for i, ((dbuf, offs, L, _), w) in enumerate(zip(views, wants)):
            whole = dbuf.cpu().numpy()
            o = offs[0]
            assert_same(whole[o:o + L], w, f"{what} bucket {i}")
            assert bool((whole[:o] == 0xEE).all()) and bool((whole[o + L:] == 0xEE).all()), i

    if not plan:
        red.sum_batched(buckets, dt, mode=MODE_ACCUM_F32)
        torch.cuda.synchronize()
        check(wants, "one_off")
        return
    p = red.make_plan(buckets, dt, mode=MODE_ACCUM_F32)
    p.launch()
    torch.cuda.synchronize()
    check(wants, "plan")
    all_ins, wants = _batch_inputs(dt, 900)       # new data at the same addresses
    for (dbuf, offs, L, bufs), ins in zip(views, all_ins):
        if L:
            dbuf[offs[0]:offs[0] + L] = 0x5A
        for b, o, x in zip(bufs, offs[1:], ins):
            if len(x):
                b[o:o + len(x)] = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize()
    p.launch()
    torch.cuda.synchronize()
    check(wants, "plan, second launch")
    p.close()


# ------------------------------------------------------------- block queue ----

BQ_BLOCKS = MIXED + [[(SMALL, 12, "cancel"), (4099, 1, "special")]]
_BQ_HOST = {}       # (dtype, seed) -> host inputs and expected bytes, shared by both shapes


class AccTable(Table):
    """test_blockq_gpu.Table whose expectations are the model's fold (and
    whose value classes include `cancel`)."""

    def host_inputs(self, seed):
        key = (int(self.dt), seed)
        if key not in _BQ_HOST:
            ins_all, wants = [], []
            for i, (dst, srcs, L, ne, n, cls) in enumerate(self.views):
                ins = am.inputs(self.dt, ne, n, cls, seed + i)
                ins_all.append(ins)
                wants.append(am.fold_bytes(ins, L, is_bf(self.dt)))
            _BQ_HOST[key] = (ins_all, wants)
        ins_all, wants = _BQ_HOST[key]
        return [[torch.from_numpy(x).pin_memory() for x in ins] for ins in ins_all], wants


@DTYPES
@pytest.mark.parametrize("shape", [0, 1], ids=["dispatch", "persistent"])
def test_blockq_release_all_two_iterations(red, dev, dt, shape):
    """make_blockq(..., MODE_ACCUM_F32): blockq_gate_kernel (wg_per_cu 0, one
    record per workgroup) and blockq_kernel (wg_per_cu 1, persistent sweep
    with the next record staged in LDS) drive run_record with OpAcc16 — the
    MIXED table of test_blockq_gpu (ragged buckets, an empty block,
    element-only buckets, 9 / 12 / 32 sources, NaN / Inf) at co-aligned
    offsets, plus a 12-source `cancel` bucket.  Everything released up front,
    two iterations on different data."""
    tab = AccTable(dev, dt, BQ_BLOCKS, offsets=True)
    q = red.make_blockq(tab.blocks, dt, MODE_ACCUM_F32)
    q.config(wg_per_cu=shape)
    for it in range(2):
        pushes, wants = tab.host_inputs(100 * it + 7)
        tab.upload(pushes)
        torch.cuda.synchronize()
        q.release(-1)
        q.launch()
        q.status()
        torch.cuda.synchronize()
        tab.check(wants)
    q.close()


# ------------------------------------------------- the mode ignored elsewhere ----

@pytest.mark.parametrize("dt,cls", [(DType.FLOAT32, "special"), (DType.INT32, "normal")],
                         ids=["FLOAT32", "INT32"])
def test_mode_ignored_by_other_dtypes(red, dev, dt, cls):
    """dtypes other than fp16 / bf16 have one arithmetic: mode = 1 gives the
    bytes of mode = 0 (NaN payload rule included for fp32)."""
    ins = am.inputs(dt, SMALL, 8, cls, 18)
    a = run_sum_n(red, dev, dt, ins, 4 * SMALL, mode=MODE_REFERENCE)
    b = run_sum_n(red, dev, dt, ins, 4 * SMALL, mode=MODE_ACCUM_F32)
    assert_same(b, a, DType(dt).name)
    assert not bool((a == 0x5A).all())


# ------------------------------------------------------------- torch operator ----

@DTYPES
def test_torch_op_sum_n_mode_1(dev, dt):
    """torch.ops.bpsr.sum_n(srcs, 1) on fp16 / bf16 tensors reaches the same
    kernels (NS = 8, VPT 1) with the mode passed through."""
    import prophet_amd.torch_ops  # noqa: F401  (registers torch.ops.bpsr.*)
    tdt = torch.bfloat16 if is_bf(dt) else torch.float16
    ins = am.inputs(dt, SMALL, 8, "cancel", 19)
    srcs = [torch.from_numpy(x.view(np.int16)).view(tdt).to(dev) for x in ins]
    out = torch.ops.bpsr.sum_n(srcs, MODE_ACCUM_F32)
    torch.cuda.synchronize()
    assert out.dtype == tdt and out.shape == srcs[0].shape
    got = out.view(torch.int16).cpu().numpy().view(np.uint8)
    assert_same(got, am.fold_bytes(ins, 2 * SMALL, is_bf(dt)), "torch op")
    ref = torch.ops.bpsr.sum_n(srcs, MODE_REFERENCE)      # and the mode does matter
    torch.cuda.synchronize()
    assert not torch.equal(ref.view(torch.int16), out.view(torch.int16))
