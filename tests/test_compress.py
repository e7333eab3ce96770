"""FP16 gradient compression without a GPU: the argument checks of the two C
calls (made before any HIP call), ``Compression`` on host tensors (torch's own
casts, the reference's path), and ``Worker`` with a compressed context against
a recording stand-in server: partitions and request word of the COMPRESSED
tensor, and every output bit equal to
``widen(div_f16(fold_f16(compress(x_r))))`` computed on the host (CPU torch
casts and ``div_``, the oracle's fp16 fold)."""
import ctypes
import threading

import numpy as np
import pytest

from oracle.oracle import PortReducer
from prophet_amd import reducer
from prophet_amd.buckets import cantor_command, depair_command
from prophet_amd.compression import (Compression, Compressor, FP16Compressor,
                                     NoneCompressor)
from prophet_amd.dtypes import DType
from prophet_amd.pushpull import ServerFrontend, Worker

torch = pytest.importorskip("torch")

A, B = 0x10000, 0x80000       # never dereferenced: every check precedes the first HIP call


@pytest.fixture(scope="module")
def lib():
    return reducer.load_library()


def test_argument_errors_without_a_gpu(lib):
    comp, decomp = lib.byteps_reduce_compress_fp16, lib.byteps_reduce_decompress_fp16
    for dt in (DType.INT32, DType.UINT8, DType.INT64, DType.FLOAT16, 7, -1):
        assert comp(A, B, 64, int(dt), None) == reducer.EDTYPE
        assert decomp(A, B, 64, int(dt), 1, None) == reducer.EDTYPE
    assert b"data type" in lib.byteps_reduce_last_error()
    for dt in (DType.FLOAT32, DType.FLOAT64, DType.BFLOAT16):
        assert comp(None, B, 64, int(dt), None) == reducer.EARGS
        assert comp(A, None, 64, int(dt), None) == reducer.EARGS
        assert decomp(None, B, 64, int(dt), 1, None) == reducer.EARGS
        assert decomp(A, B, 64, int(dt), 0, None) == reducer.EARGS
        assert decomp(A, B, 64, int(dt), -3, None) == reducer.EARGS
        # nothing to do: no launch, no pointer needed
        assert comp(None, None, 0, int(dt), None) == reducer.OK
        assert decomp(None, None, 0, int(dt), 4, None) == reducer.OK
    assert comp(A, B, ctypes.c_size_t(-1).value // 2, int(DType.FLOAT64), None) == reducer.EARGS


def test_any_overlap_is_rejected(lib):
    comp, decomp = lib.byteps_reduce_compress_fp16, lib.byteps_reduce_decompress_fp16
    f32 = int(DType.FLOAT32)
    n = 100                                    # fp16: 200 bytes, f32: 400 bytes
    assert comp(A, A, n, f32, None) == reducer.EARGS              # the same start
    assert comp(A + 399, A, n, f32, None) == reducer.EARGS        # dst's first byte = src's last
    assert comp(A, A + 199, n, f32, None) == reducer.EARGS        # src's first byte = dst's last
    assert comp(A + 100, A, n, f32, None) == reducer.EARGS        # dst inside src
    assert decomp(A, A, n, f32, 1, None) == reducer.EARGS
    assert decomp(A, A + 399, n, f32, 1, None) == reducer.EARGS
    assert decomp(A + 199, A, n, f32, 1, None) == reducer.EARGS
    assert b"overlap" in lib.byteps_reduce_last_error()


def test_reducer_bounds_check_precedes_the_call():
    red = reducer.GpuReducer()
    half = torch.empty(99, dtype=torch.float16)
    wide = torch.empty(100, dtype=torch.float32)
    with pytest.raises(ValueError):
        red.compress_fp16(half, wide, 100, DType.FLOAT32)           # dst one element short
    with pytest.raises(ValueError):
        red.decompress_fp16(wide, half, 100, DType.FLOAT32)         # src one element short
    with pytest.raises(ValueError):
        red.decompress_fp16(wide[:99], torch.empty(100, dtype=torch.float16), 100,
                            DType.FLOAT32, 2)                       # dst one element short
    with pytest.raises(ValueError):
        red.compress_fp16(torch.empty(100, dtype=torch.float16), wide, 100, DType.FLOAT64)


def test_compression_interface_on_host_tensors():
    assert Compression.none is NoneCompressor and Compression.fp16 is FP16Compressor
    assert issubclass(FP16Compressor, Compressor)
    x = torch.randn(1000)
    c, ctx = Compression.none.compress(x)
    assert c is x and ctx is None and Compression.none.decompress(c, ctx) is x
    for dt in (torch.float32, torch.float64, torch.bfloat16):
        x = torch.randn(1000).to(dt)
        c, ctx = Compression.fp16.compress(x)
        assert ctx == dt and c.dtype == torch.float16
        assert torch.equal(c.view(torch.int16), x.to(torch.float16).view(torch.int16))
        back = Compression.fp16.decompress(c, ctx)
        assert back.dtype == dt and torch.equal(back, c.to(dt))
    for x in (torch.arange(10), torch.arange(10, dtype=torch.uint8), torch.randn(10).half()):
        c, ctx = Compression.fp16.compress(x)
        assert c is x and ctx == x.dtype                 # untouched, the same object
        assert Compression.fp16.decompress(c, ctx) is x
    a = np.linspace(-3, 3, 77, dtype=np.float32)
    c, ctx = Compression.fp16.compress(a)
    assert isinstance(c, np.ndarray) and c.dtype == np.float16 and ctx == np.float32
    assert np.array_equal(c.view(np.uint16),
                          torch.from_numpy(a).to(torch.float16).numpy().view(np.uint16))
    back = Compression.fp16.decompress(c, ctx)
    assert back.dtype == np.float32 and np.array_equal(back, c.astype(np.float32))
    ai = np.arange(5)
    assert Compression.fp16.compress(ai)[0] is ai


def test_f64_is_rounded_through_f32():
    # 1 + 2^-11 is the midpoint of two fp16 values (ties to even: 1.0); the
    # 2^-30 tips a DIRECT f64 -> f16 rounding up to 1 + 2^-10, but is lost in
    # the f32 step the host conversion takes first
    x = torch.tensor([1 + 2.0 ** -11 + 2.0 ** -30, -(1 + 2.0 ** -11 + 2.0 ** -30)],
                     dtype=torch.float64)
    c, ctx = Compression.fp16.compress(x)
    assert ctx == torch.float64
    assert c.view(torch.int16).tolist() == [0x3c00, 0xbc00 - 0x10000]
    direct = x.numpy().astype(np.float16)
    assert direct.view(np.uint16).tolist() == [0x3c01, 0xbc01]      # what it must NOT be


def test_decompress_into_divides_before_widening():
    h = torch.from_numpy(np.arange(1 << 16, dtype=np.uint16).view(np.float16))
    fin = ~torch.isnan(h)
    for dt in (torch.float32, torch.float64, torch.bfloat16):
        out = torch.empty(h.numel(), dtype=dt)
        assert Compression.fp16.decompress_into(out, h, 3) is out
        want = h.clone().div_(3).to(dt)
        assert torch.equal(out[fin], want[fin]) and bool(torch.isnan(out[~fin]).all())
    after = (h.to(torch.float32) / 3)                   # the wrong order: widen, then divide
    out = Compression.fp16.decompress_into(torch.empty(h.numel()), h, 3)
    assert int((out[fin] != after[fin]).sum()) == 42344
    with pytest.raises(ValueError):
        Compression.fp16.decompress_into(out, h, 0)


class RecordingServer:
    """Stand-in server for a compressed context: records every push
    (key, worker, bytes, dtype); once all workers pushed a key, its store
    becomes the last push (init round) or the oracle's fp16 left fold of the
    pushes in arrival order, which it also records per round."""

    def __init__(self, n_workers):
        self.n = n_workers
        self.cv = threading.Condition()
        self.port = PortReducer(nthreads=1)
        self.store, self.pending, self.inited = {}, {}, set()
        self.log, self.orders = [], {}

    def push(self, key, worker, data, dtype, nbytes=None):
        raw = np.asarray(data).view(np.uint8).copy()
        assert nbytes == raw.nbytes
        with self.cv:
            self.log.append((key, worker, nbytes, int(dtype)))
            self.pending.setdefault(key, []).append((worker, raw))
            if len(self.pending[key]) == self.n:
                arrived = self.pending.pop(key)
                if key not in self.inited:
                    self.store[key] = arrived[-1][1]
                    self.inited.add(key)
                else:
                    out = np.zeros(nbytes, np.uint8)
                    assert self.port.sum_n(out, [b for _, b in arrived], nbytes,
                                           DType.FLOAT16) == 0
                    self.store[key] = out
                    self.orders.setdefault(key, []).append([w for w, _ in arrived])
                self.cv.notify_all()
            elif key not in self.inited:
                self.cv.wait_for(lambda: key in self.inited)     # init barrier

    def pull(self, key, out, nbytes=None):
        with self.cv:
            self.cv.wait_for(lambda: key not in self.pending)
            np.asarray(out).view(np.uint8)[:] = self.store[key]


def _values(rank, n):
    rng = np.random.default_rng(77 + rank)
    x = rng.standard_normal(n).astype(np.float32)
    x[:8] = [65504.0, -65520.0, 7e4, 1e-7, -3e-8, 0.0, -0.0, 6.1e-5][:8]   # past max, subnormal
    return x


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("average", [True, False])
def test_worker_pushes_the_compressed_tensor(kind, average):
    N, n = 2, 2 * 500 + 77
    srv = RecordingServer(N)
    fe = ServerFrontend(srv, size=N)
    ws = [Worker(r, fe, partition_bytes=1000) for r in range(N)]
    xs = [_values(r, n) for r in range(N)]
    wrap = (lambda a: a) if kind == "numpy" else torch.from_numpy
    ins = [wrap(x.copy()) for x in xs]
    outs = [wrap(np.full(n, 123.0, np.float32)) for _ in range(N)]
    errors = []

    def run(w):
        try:
            w.declare("g")
            ctx = w.init_tensor("g", wrap(np.zeros(n, np.float32)), DType.FLOAT32,
                                compression=Compression.fp16)
            assert ctx.dtype == DType.FLOAT16 and ctx.size == 2 * n
            w.push_pull("g", ins[w.rank], output=outs[w.rank], average=average)
        except Exception as e:  # surfaced below
            errors.append(repr(e))
    ts = [threading.Thread(target=run, args=(w,)) for w in ws]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=30)
    assert not errors, errors
    c = ws[0].contexts["g"]
    assert [ln for _, _, ln in c.parts] == [1000, 1000, 154]
    assert c.key_list == [0, 1, 2]
    # the request word the front end decoded carried FLOAT16, for init and data pushes alike
    assert len(srv.log) == 2 * N * 3
    assert all(dt == DType.FLOAT16 for _, _, _, dt in srv.log)
    assert depair_command(cantor_command(0, c.dtype)) == (0, DType.FLOAT16)
    halves = [torch.from_numpy(x).to(torch.float16).numpy().view(np.uint8) for x in xs]
    for r in range(N):                                  # the input is left as it was
        assert np.array_equal(np.asarray(ins[r]).view(np.uint32), xs[r].view(np.uint32))
    for key, off, ln in c.parts:
        (order,) = srv.orders[key]
        assert sorted(order) == list(range(N))
        folded = np.zeros(ln, np.uint8)
        srv.port.sum_n(folded, [halves[r][off:off + ln].copy() for r in order], ln,
                       DType.FLOAT16)
        q = torch.from_numpy(folded.view(np.float16).copy())
        if average:
            q.div_(N)
        want = q.to(torch.float32).numpy()
        assert not np.isnan(want).any()
        for r in range(N):
            got = np.asarray(outs[r])[off // 2:(off + ln) // 2]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (key, r)


def test_none_keeps_the_uncompressed_context_and_broadcast_refuses_fp16():
    srv = RecordingServer(1)
    w = Worker(0, ServerFrontend(srv, size=1), partition_bytes=1000)
    x = np.arange(300, dtype=np.float32)
    w.declare("p")
    c = w.init_tensor("p", x, DType.FLOAT32, compression=Compression.none)
    assert c.compressor is None and c.size == 1200 and c.dtype == DType.FLOAT32
    assert [ln for _, _, ln in c.parts] == [1000, 200]
    w.declare("h")
    h = np.arange(300, dtype=np.float16)
    ch = w.init_tensor("h", h, DType.FLOAT16, compression=Compression.fp16)
    assert ch.compressor is None and ch.size == 600            # fp16 passes through
    w.declare("g")
    w.init_tensor("g", x, DType.FLOAT32, compression=Compression.fp16)
    with pytest.raises(ValueError):
        w.broadcast("g", x, root_rank=0)
    with pytest.raises(ValueError):
        w.push_pull("g", np.arange(300, dtype=np.float64))     # not the declared tensor
