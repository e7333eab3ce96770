"""Reference mode (the parity claim) at the tile sizes real folds run: 8 KiB
and 16 KiB tiles, VPT 2 and 4 (bpsr_internal.h fold_vpt keeps them from 2,048
tiles on), with NaNs that reach the exact replay — on fold_kernel,
batched_kernel, blockq_gate_kernel and blockq_kernel, every comparison on the
raw bytes against oracle.oracle.PortReducer, with no tolerance.

What only a tile of more than one vector per lane can get wrong:
  * fold_tile_full_buf replays slot j at byte0 + voff + j * kBlock * 16: a
    replay that re-read slot 0 is correct at VPT 1;
  * fold_tile_body (the guarded partial tile) replays at off0 + j * kStep
    and carries valid[j] per slot: in V2's partial tile slot 1 is valid on lanes 0..43 only, in
    V4's slot 2 on lanes 0..187 and slot 3 nowhere;
  * NS = 16 at VPT 4 takes two load groups (G = 8);
  * the f64, i8 / u8, i32 and i64 instantiations at VPT 2 and 4.

tests/fold_shapes.py has the shapes and the inputs (order_probe's probes in
the first, an interior and the last full tile, the partial tile, the head and
the tail; finite tiles between them); tests/test_fold_shapes.py checks on the
CPU that every case gets the tile size, kernel and policy its id names, and
that a replay at the wrong slot or in the wrong order changes bytes in every
probed tile.  dst is prefilled with 0x5A, 0xEE guard bytes lie around dst and
every source, and no source may change (fold_run.Operands).
"""
import pytest

import fold_shapes as fs
from fold_run import Operands, assert_elements
from prophet_amd.dtypes import DType, elem_size
from test_blockq_gpu import MIXED, Table

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

MODE_REFERENCE = 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def red(dev):
    from prophet_amd.reducer import GpuReducer
    return GpuReducer(device=0)


def dtype_ids(dts):
    return pytest.mark.parametrize("dt", dts, ids=lambda d: DType(d).name)


# -------------------------------------------------------------------- sum_n ----

def check_sum_n(red, dev, case, inplace=False):
    """One byteps_reduce_sum_n of fold_shapes.fold_case(case) against the
    oracle's bytes."""
    dt, n, shape = case[:3]
    off = case[3] if len(case) > 3 else 0
    ins, kind, want, _ = fs.fold_case(dt, n, shape, off)
    L = len(want)
    ops = Operands(dev, n, L, [off] * n, 16 + off, inplace).load(ins)
    torch.cuda.synchronize()
    red.sum_n(ops.dst, ops.srcs, L, dt, mode=MODE_REFERENCE)
    torch.cuda.synchronize()
    assert_elements(dt, ops.result(), want, kind,
                    fs.case_id(case) + (" in place" if inplace else ""))


@pytest.mark.parametrize("case", fs.SUM_N, ids=fs.case_id)
def test_sum_n_separate_dst(red, dev, case):
    """fold_kernel<Op, VPT 2 | 4, kPolWt, NS 2 | 8 | 16 | generic>: 2,047 full
    tiles (fold_tile_full_buf), the guarded partial tile (fold_tile_body) and
    the tail (fold_elements; fp16: the scalar tail).  (n, V4) with n > 4 gets
    VPT 4 from fold_vpt's mid-size rule, n <= 4 from tuning_for_n."""
    check_sum_n(red, dev, case)


@pytest.mark.parametrize("case", fs.IN_PLACE, ids=fs.case_id)
def test_sum_n_in_place(red, dev, case):
    """dst is srcs[0]: the replay of slot j re-reads srcs[0] from memory,
    which the same lane overwrites afterwards, slot by slot."""
    check_sum_n(red, dev, case, inplace=True)


@pytest.mark.parametrize("case", fs.OFFSET, ids=fs.case_id)
def test_sum_n_coaligned_byte_offset(red, dev, case):
    """Every operand at the same byte offset inside its 16-byte line: head
    elements through fold_elements and a non-zero vec_off under the tiles'
    offsets (floats: 8 bytes; i32: 4)."""
    check_sum_n(red, dev, case)


# -------------------------------------------------- sum_batched and make_plan ----

_TABLE_HOST = {}        # (dtype, vpt, seed) -> fold_shapes.table_inputs, shared


def table_host(dt, vpt, seed, dups=None):
    key = (int(dt), vpt, seed, bool(dups))
    if key not in _TABLE_HOST:
        _TABLE_HOST[key] = fs.table_inputs(dt, fs.table_spec(dt, vpt), vpt, seed, dups)
    return _TABLE_HOST[key]


def check_batched(red, dev, dt, vpt, plan, dups=None):
    """The ragged table of fold_shapes.table_spec(dt, vpt) as a one-off launch
    or as a plan, launched a second time on refilled data.  `dups`: bucket
    index -> groups of sources that are one buffer (fold_shapes.TABLE_DUPS)."""
    spec = fs.table_spec(dt, vpt)
    host = table_host(dt, vpt, 300, dups)
    ops = []
    for i, ((ne, n, offs, _), (ins, _, want)) in enumerate(zip(spec, host)):
        o = fs.bucket_offsets(offs, n)
        ops.append(Operands(dev, n, len(want), o[1:], o[0],
                            same=(dups or {}).get(i, ())).load(ins))
    buckets = [o.bucket for o in ops]

    def check(host, what):
        for i, (o, (_, kind, want)) in enumerate(zip(ops, host)):
            assert_elements(dt, o.result(), want, kind, f"{what} bucket {i}")

    torch.cuda.synchronize()
    if not plan:
        red.sum_batched(buckets, dt, mode=MODE_REFERENCE)
        torch.cuda.synchronize()
        check(host, "one_off")
        return
    p = red.make_plan(buckets, dt, mode=MODE_REFERENCE)
    p.launch()
    torch.cuda.synchronize()
    check(host, "plan")
    host = table_host(dt, vpt, 900, dups)   # new data at the same addresses
    for o, (ins, _, _) in zip(ops, host):
        o.load(ins)
    torch.cuda.synchronize()
    p.launch()
    torch.cuda.synchronize()
    check(host, "plan, second launch")
    p.close()


@dtype_ids(fs.BATCH_DTYPES)
@pytest.mark.parametrize("vpt", [2, 4], ids=["vpt2", "vpt4"])
@pytest.mark.parametrize("plan", [False, True], ids=["one_off", "plan"])
def test_batched_ragged_table_big_tiles(red, dev, dt, vpt, plan):
    """batched_kernel<Op, VPT 2 | 4> (run_record): the ragged table of
    test_parity_gpu.test_batched_ragged_mixed_table, order probes in the float
    buckets, plus a two-source ballast bucket of 2,047 full tiles that brings
    the table's vector count to VPT 2 (nmax = 32: tuned 2) or VPT 4 (the
    mid-size rule).  The small buckets then are kTileFull and kTilePartial
    records of the big tile, on the register path (NS = -8) and on the
    pointer-array path (9, 12 and 32 sources)."""
    check_batched(red, dev, dt, vpt, plan)


# ------------------------------------------------------------- block queue ----

_BQ_HOST = {}           # (dtype, vpt, seed) -> host inputs, kinds, expected bytes


class ProbeTable(Table):
    """test_blockq_gpu.Table with guard bytes around every operand, the byte
    offsets the ragged table gives the same buckets, order probes in the
    float buckets (placed for tiles of 256 * vpt vectors) and the oracle's
    fold as the expectation."""

    def __init__(self, dev, dt, blocks, vpt, dups=None):
        self.dt, self.es, self.vpt = dt, elem_size(dt), vpt
        self.dups = dups or {}      # bucket index -> groups of sources in one buffer
        self.blocks, self.views, self.ops, self.offs = [], [], [], []
        for blk in blocks:
            out = []
            for ne, n, cls in blk:
                offs = fs.blockq_offsets(dt, ne, n)
                o = fs.bucket_offsets(offs, n)
                ops = Operands(dev, n, ne * self.es, o[1:], o[0],
                               same=self.dups.get(len(self.ops), ()))
                out.append(ops.bucket)
                self.ops.append(ops)
                self.offs.append(offs)
                self.views.append((ops.dst_view, ops.src_views, ops.L, ne, n, cls))
            self.blocks.append(out)

    def host_inputs(self, seed):
        key = (int(self.dt), self.vpt, seed, bool(self.dups))
        if key not in _BQ_HOST:
            rows = []
            for i, ((_, _, L, ne, n, cls), offs) in enumerate(zip(self.views, self.offs)):
                reg = fs.bucket_regions(self.dt, ne, offs, n, self.vpt)
                ins, kind = fs.probe_inputs(self.dt, ne, n, seed + i, reg, cls)
                ins = fs.share(ins, self.dups.get(i, ()))
                rows.append((ins, kind, fs.oracle_fold(self.dt, ins, L)))
            _BQ_HOST[key] = rows
        rows = _BQ_HOST[key]
        self.kinds = [k for _, k, _ in rows]
        pinned = [[torch.from_numpy(x).pin_memory() for x in ins] for ins, _, _ in rows]
        return ([fs.share(ps, self.dups.get(i, ())) for i, ps in enumerate(pinned)],
                [w for _, _, w in rows])

    def upload(self, pushes, stream=None):
        for ops, ps in zip(self.ops, pushes):
            ops.load(ps)

    def check(self, wants):
        for i, (ops, w) in enumerate(zip(self.ops, wants)):
            assert_elements(self.dt, ops.result(), w, self.kinds[i], f"bucket {i}")


def check_blockq(red, dev, dt, shape, vpt, iterations, dups=None):
    """Everything released up front, `iterations` launches on different data."""
    tab = ProbeTable(dev, dt, MIXED, vpt, dups)
    q = red.make_blockq(tab.blocks, dt, MODE_REFERENCE)
    q.config(wg_per_cu=shape)
    for it in range(iterations):
        pushes, wants = tab.host_inputs(100 * it + 7)
        tab.upload(pushes)
        torch.cuda.synchronize()
        q.release(-1)
        q.launch()
        q.status()
        torch.cuda.synchronize()
        tab.check(wants)
    q.close()


@dtype_ids(fs.BLOCKQ_DTYPES)
@pytest.mark.parametrize("vpt", [2, 4], ids=["vpt2", "vpt4"])
@pytest.mark.parametrize("shape", [0, 1], ids=["dispatch", "persistent"])
def test_blockq_big_tiles_two_iterations(red, dev, monkeypatch, dt, vpt, shape):
    """blockq_gate_kernel (one record per workgroup) and blockq_kernel (the
    persistent sweep) at VPT 2 and 4 through BPSR_BQ_VPT, which every create
    reads: test_blockq_gpu's MIXED table (ragged buckets, an empty block,
    element-only buckets, 9 / 12 / 32 sources) at co-aligned offsets, order
    probes in the float buckets."""
    monkeypatch.setenv("BPSR_BQ_VPT", str(vpt))
    check_blockq(red, dev, dt, shape, vpt, 2)
