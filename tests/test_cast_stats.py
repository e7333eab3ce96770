"""Decompress statistics on the host: ``decompress_into(..., stats=)`` and
``decompress_many_into(..., stats=)`` of the cast compressors follow the
pinned definition (``compression.decompress_stats``: the f64 sum of the
squares of the finite values written, the count of the others) for numpy
arrays and CPU tensors, both wires, divisors 1 and 8; a ``stats`` of the wrong
dtype, shape or device is refused; and ``Worker.grad_stats`` over a
host-resident 2-worker round.  No GPU."""
import threading

import numpy as np
import pytest

from prophet_amd.compression import Compression, decompress_stats
from prophet_amd.dtypes import DType
from prophet_amd.pushpull import GradStats, ServerFrontend, Worker

torch = pytest.importorskip("torch")

WIRES = [("fp16", Compression.fp16), ("bf16", Compression.bf16),
         ("fp16_ef", Compression.fp16_ef), ("bf16_sr", Compression.bf16_sr)]


def _wire_values(name, n, seed):
    """n wire values as a CPU tensor of the wire dtype: random, with +-inf,
    NaN, zeros, the format's largest value and a subnormal mixed in."""
    dt = torch.float16 if name.startswith("fp16") else torch.bfloat16
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, generator=g) * 100).to(dt)
    fi = torch.finfo(dt)
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), 0.0, -0.0, fi.max, -fi.max,
                            fi.tiny / 4, 60000.0 if dt == torch.float16 else 3e38]).to(dt)
    x[:special.numel()] = special[:n]
    return x[torch.randperm(n, generator=g)]


def _definition(out):
    """The issue's three numpy lines, written out independently."""
    x = (out.to(torch.float64).numpy() if hasattr(out, "data_ptr") else out.astype(np.float64))
    x = x.reshape(-1)
    fin = np.isfinite(x)
    return np.square(x[fin]).sum(), np.count_nonzero(~fin)


def _as_numpy_wire(w):
    return w.view(torch.int16).numpy().view(np.uint16) if w.dtype == torch.bfloat16 else w.numpy()


@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("name,comp", WIRES)
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_decompress_into_reports_the_definition(name, comp, divisor, kind):
    for wide in (torch.float32, torch.float64):
        w = _wire_values(name, 1000, seed=3)
        plain = torch.empty(1000, dtype=wide)
        comp.decompress_into(plain, w, divisor)
        if kind == "numpy":
            out = np.empty(1000, dtype=plain.numpy().dtype)
            st = np.full(2, np.nan)
            comp.decompress_into(out, _as_numpy_wire(w), divisor, stats=st)
            got = out
        else:
            out = torch.empty(1000, dtype=wide)
            st = torch.full((2,), float("nan"), dtype=torch.float64)
            comp.decompress_into(out, w, divisor, stats=st)
            got = out.numpy()
        # the bytes are the plain decompress's
        assert got.tobytes() == plain.numpy().tobytes()
        ss, nf = _definition(plain)
        assert nf >= 3 and ss > 0
        assert float(st[0]) == ss and float(st[1]) == nf
        assert decompress_stats(plain) == (ss, nf)


def test_overflow_under_the_divide():
    """60000 / 8 stays finite, inf / 8 does not; on the fp16 wire 60000 is
    finite and counts 3.6e9 towards the sum."""
    w = torch.tensor([60000.0, float("inf"), 2.0], dtype=torch.float16)
    out = torch.empty(3)
    st = torch.empty(2, dtype=torch.float64)
    Compression.fp16.decompress_into(out, w, 8, stats=st)
    assert st.tolist() == [7500.0 ** 2 + 0.25 ** 2, 1.0]
    Compression.fp16.decompress_into(out, w, 1, stats=st)
    assert st.tolist() == [60000.0 ** 2 + 4.0, 1.0]


@pytest.mark.parametrize("divisor", [1, 8])
@pytest.mark.parametrize("name,comp", WIRES)
def test_decompress_many_into_rows_follow_outs(name, comp, divisor):
    sizes = [5, 0, 1, 300, 2049]
    ws = [_wire_values(name, n, seed=10 + i) for i, n in enumerate(sizes)]
    for kind in ("numpy", "torch"):
        if kind == "numpy":
            outs = [np.empty(n, np.float32) for n in sizes]
            st = np.full((len(sizes), 2), np.nan)
            comp.decompress_many_into(outs, [_as_numpy_wire(w) for w in ws], divisor, stats=st)
        else:
            outs = [torch.empty(n) for n in sizes]
            st = torch.full((len(sizes), 2), float("nan"), dtype=torch.float64)
            comp.decompress_many_into(outs, ws, divisor, stats=st)
        for i, (o, w) in enumerate(zip(outs, ws)):
            plain = torch.empty(sizes[i])
            comp.decompress_into(plain, w, divisor)
            assert np.asarray(o).tobytes() == plain.numpy().tobytes()
            ss, nf = _definition(plain)
            assert float(st[i][0]) == ss and float(st[i][1]) == nf, (kind, i)
        assert float(st[1][0]) == 0.0 and float(st[1][1]) == 0.0     # the empty tensor's row


def test_stats_argument_errors():
    comp = Compression.fp16
    w = torch.ones(4, dtype=torch.float16)
    out = torch.empty(4)
    for bad in (torch.empty(2), np.empty(2, np.float32), [0.0, 0.0], torch.empty(2).long()):
        with pytest.raises(ValueError, match="float64"):                  # dtype
            comp.decompress_into(out, w, 1, stats=bad)
    for bad in (torch.empty(3, dtype=torch.float64), np.empty((1, 2)), np.empty((2, 1))):
        with pytest.raises(ValueError, match="shape"):
            comp.decompress_into(out, w, 1, stats=bad)
    for bad in (np.empty(4), np.empty((3, 2)), torch.empty((2, 3), dtype=torch.float64)):
        with pytest.raises(ValueError, match="shape"):
            comp.decompress_many_into([out, out.clone()], [w, w], 1, stats=bad)
    with pytest.raises(ValueError, match="float64"):
        comp.decompress_many_into([out], [w], 1, stats=np.empty((1, 2), np.float32))

    class OnDevice:
        """A float64 tensor that says it lives on a GPU: the device check
        comes before anything is computed."""
        dtype, shape, device = torch.float64, (2,), torch.device("cuda", 0)

        def data_ptr(self):
            return 0

        def reshape(self, *s):
            return self

    with pytest.raises(ValueError, match="on the host"):
        comp.decompress_into(out, w, 1, stats=OnDevice())
    many = OnDevice()
    many.shape = (1, 2)
    with pytest.raises(ValueError, match="on the host"):
        comp.decompress_many_into([out], [w], 1, stats=many)
    # a null plan is refused by the library before any device call
    from prophet_amd import reducer
    lib = reducer.load_library()
    assert lib.byteps_reduce_cast_plan_decompress_stats(None, 1, None, None) == reducer.EARGS
    assert b"null plan" in lib.byteps_reduce_last_error()


class SummingServer:
    """A host server of two workers: a pull returns the sum, in the request's
    dtype, of the round's two pushes."""

    TORCH = {int(DType.FLOAT32): torch.float32, int(DType.FLOAT16): torch.float16,
             int(DType.BFLOAT16): torch.bfloat16}

    def __init__(self):
        self.cv = threading.Condition()
        self.me = threading.local()           # a worker pushes and pulls on one thread
        self.pending, self.result, self.round, self.want = {}, {}, {}, {}

    def push(self, key, worker, data, dtype, nbytes=None):
        raw = np.asarray(data).view(np.uint8).copy()
        self.me.rank = worker
        with self.cv:
            # the init push is a barrier: a worker's next push of the key waits
            # for the round its last one belongs to
            assert self.cv.wait_for(lambda: worker not in self.pending.get(key, {}), timeout=30)
            p = self.pending.setdefault(key, {})
            p[worker] = torch.from_numpy(raw).view(self.TORCH[int(dtype)])
            self.want[(key, worker)] = self.round.get(key, 0) + 1
            if len(p) == 2:
                self.result[key] = (p[0] + p[1]).view(torch.uint8).numpy().copy()
                self.pending[key] = {}
                self.round[key] = self.round.get(key, 0) + 1
                self.cv.notify_all()

    def pull(self, key, out, nbytes=None):
        with self.cv:
            want = self.want[(key, self.me.rank)]
            assert self.cv.wait_for(lambda: self.round.get(key, 0) >= want, timeout=30)
            np.asarray(out).view(np.uint8)[:] = self.result[key]


def test_grad_stats_over_a_two_worker_round_on_the_host():
    n = 500
    names = ["plain", "a16", "bef", "sr16"]
    comps = [Compression.none, Compression.fp16, Compression.bf16_ef, Compression.fp16_sr]
    rng = np.random.default_rng(5)
    grads = [{k: rng.standard_normal(n).astype(np.float32) * 10 for k in names} for _ in range(2)]
    for r in range(2):
        grads[r]["a16"][7] = 40000.0          # 40000 + 40000 is inf in fp16
    server = SummingServer()
    outs, stats, errors = [None, None], [None, None], []

    def run(rank):
        try:
            w = Worker(rank, ServerFrontend(server, size=2), sr_seed=1)
            for k in names:
                w.declare(k)
            for k, c in zip(names, comps):
                w.init_tensor(k, grads[rank][k].copy(), DType.FLOAT32, compression=c)
            assert w.grad_stats is None
            x = {k: v.copy() for k, v in grads[rank].items()}
            w.push_pull_iteration(x, average=True, stats=True)
            outs[rank], stats[rank] = x, w.grad_stats
            # the single-tensor call: one row; an uncompressed context: none
            y = grads[rank]["bef"].copy()
            w.push_pull("bef", y, average=True, stats=True)
            assert w.grad_stats.names == ["bef"] and w.grad_stats.skipped == []
            assert tuple(w.grad_stats.rows.shape) == (1, 2)
            ss, nf = _definition(y)
            assert float(w.grad_stats["bef"][0]) == ss and float(w.grad_stats["bef"][1]) == nf
            z = grads[rank]["plain"].copy()
            w.push_pull("plain", z, stats=True)
            assert w.grad_stats.names == [] and w.grad_stats.skipped == ["plain"]
            assert tuple(w.grad_stats.rows.shape) == (0, 2)
            w.close()
        except Exception as e:                # noqa: BLE001 — reported by the main thread
            errors.append(e)
            raise

    ts = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not errors, errors
    for rank in range(2):
        gs = stats[rank]
        assert isinstance(gs, GradStats)
        assert gs.names == ["a16", "bef", "sr16"] and gs.skipped == ["plain"]
        assert isinstance(gs.rows, np.ndarray) and gs.rows.shape == (3, 2)
        assert gs.rows.dtype == np.float64
        total, bad = 0.0, 0
        for i, k in enumerate(gs.names):
            ss, nf = _definition(outs[rank][k])
            assert gs.rows[i, 0] == ss and gs.rows[i, 1] == nf, k
            assert gs[k][0] == ss and gs[k][1] == nf
            total, bad = total + ss, bad + nf
        assert gs["a16"][1] == 1 and np.isinf(outs[rank]["a16"][7])
        assert gs.nonfinite() == bad == 1
        assert gs.sumsq() == pytest.approx(total, rel=1e-15)
        assert gs.norm() == pytest.approx(total ** 0.5, rel=1e-15)
    # both workers were delivered the same aggregate
    for k in ("a16", "bef"):
        assert np.array_equal(outs[0][k].view(np.uint32), outs[1][k].view(np.uint32))
