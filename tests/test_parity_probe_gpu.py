"""Reference mode (the headline mode) of the direct calls on the order probes
of tests/order_probe.py: byteps_reduce_sum_n against the oracle's left fold in
the caller's source order, on the raw bytes, with no tolerance.

The probes put NaNs with a payload per source, inf / -inf clashes, -0,
subnormals and +-(largest finite) at every third element of the first tile,
the last full tile and the partial tile, and at every element of the head and
the ragged tail — so every vector there goes to the exact replay
(fold_vector_exact) beside finite lanes that must still match, fold_elements
sees NaNs in the head, behind the last vector and in fp16's scalar tail
(tail_sem_from: any NaN is 0x7fff), and a replay or a fast path that took the
sources in another order, or an accumulator not started from srcs[0], changes
bytes (tests/test_order_probe.py shows that on the CPU).  run_sum_n (of
test_accum_gpu) adds 0xEE guard bytes on both sides of dst, the sources left
unchanged, and the in-place form.

Geometry as in test_accum_gpu: VPT 1 at these sizes, a tile is 4 KiB per
operand; the shape is 3 full tiles, 100 vectors and a ragged tail."""
import pytest

import order_probe as op
from oracle.oracle import PortReducer
from prophet_amd.dtypes import DType, elem_size
from test_accum_gpu import MODE_REFERENCE, run_sum_n

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dt", op.DIRECT_DTYPES, ids=lambda d: DType(d).name)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def red(dev):
    from prophet_amd.reducer import GpuReducer
    return GpuReducer(device=0)


@pytest.fixture(scope="module")
def port():
    return PortReducer(nthreads=4)


def check(dt, got, want, kind, what):
    """Raw bytes; a mismatch names the first elements and their probe kinds."""
    bad = op.changed(dt, got, want).nonzero()[0]
    if len(bad):
        U = op.bits_type(dt)
        g, w = got.view(U), want.view(U)
        raise AssertionError(
            f"{what}: {len(bad)} of {len(w)} elements differ; first "
            + ", ".join(f"[{i}] kind {int(kind[i])} got {int(g[i]):#x} want {int(w[i]):#x}"
                        for i in bad[:6]))


@DTYPES
@pytest.mark.parametrize("n", op.DIRECT_N)
def test_sum_n_source_counts(red, dev, port, dt, n):
    """fold_kernel's compile-time source counts NS = 2, 8, 16, the generic
    kernel (n = 3, 9, 32) and the chain of 40 (32 sources, then [result] + 8
    in place), separate dst."""
    ins, kind, ne, _ = op.direct_inputs(dt, n)
    L = ne * elem_size(dt)
    got = run_sum_n(red, dev, dt, ins, L, mode=MODE_REFERENCE)
    check(dt, got, op.fold(port, dt, ins, range(n)), kind, f"n={n}")


@DTYPES
@pytest.mark.parametrize("n", op.DIRECT_N_IN_PLACE)
def test_sum_n_in_place(red, dev, port, dt, n):
    """dst is srcs[0]: the replay re-reads srcs[0] from memory, which the
    same thread overwrites afterwards; 40 sources chain in place."""
    ins, kind, ne, _ = op.direct_inputs(dt, n)
    L = ne * elem_size(dt)
    got = run_sum_n(red, dev, dt, ins, L, inplace=True, mode=MODE_REFERENCE)
    check(dt, got, op.fold(port, dt, ins, range(n)), kind, f"in place n={n}")


@pytest.mark.parametrize("n", [8, 9])
@pytest.mark.parametrize("dt,off", [(dt, off) for dt, offs in op.DIRECT_OFFSETS.items()
                                    for off in offs],
                         ids=lambda v: DType(v).name if isinstance(v, DType) else str(v))
def test_sum_n_coaligned_byte_offsets(red, dev, port, dt, off, n):
    """Every operand at the same byte offset inside its 16-byte line: fp16 at
    2, 6 and 14 (a head of 7, 5 or 1 elements); none of those is
    element-aligned for fp32, which takes 4 and 12 (a head of 3 or 1).  The
    head and the elements behind the last whole vector go through
    fold_elements, around vector tiles (NS = 8 and generic).  fp16 has
    n % 8 = 3 here (order_probe.ragged_key): the heads of 7 and 5 leave body
    elements and the scalar tail behind the last vector, the head of 1 puts
    the scalar tail's first element inside the last vector.  Head, body rest
    and scalar tail each begin with an `all` probe."""
    es = elem_size(dt)
    assert off % es == 0
    head = (16 - off) // es
    ins, kind, ne, _ = op.direct_inputs(dt, n, head)
    L = ne * es
    got = run_sum_n(red, dev, dt, ins, L, src_offs=[off] * n, dst_off=16 + off,
                    mode=MODE_REFERENCE)
    check(dt, got, op.fold(port, dt, ins, range(n)), kind, f"off={off} n={n}")


@DTYPES
def test_sum_n_not_coaligned_operands(red, dev, port, dt):
    """Operands at different offsets, the last not even element-aligned (the
    offsets of test_parity_gpu.test_not_coaligned_and_unaligned): the whole
    bucket is element work, byte-wise loads and stores."""
    es = elem_size(dt)
    ins, kind, ne, _ = op.element_path_inputs(dt)
    got = run_sum_n(red, dev, dt, ins, ne * es, src_offs=[0, es, 3 * es, 1], dst_off=5,
                    mode=MODE_REFERENCE)
    check(dt, got, op.fold(port, dt, ins, range(4)), kind, "element path")
