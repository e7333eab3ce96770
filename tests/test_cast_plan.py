"""Cast plans without a GPU: the argument checks of byteps_reduce_cast_plan_*
(all made before any HIP call), the host-side bounds check of ``CastPlan``,
``compress_many_into`` / ``decompress_many_into`` on host tensors against the
per-tensor calls, and ``push_pull_iteration(average=True)`` with compressed
and uncompressed contexts against per-tensor ``push_pull(average=True)``, over
the recording stand-in server of tests/test_compress.py."""
import ctypes
import threading

import numpy as np
import pytest

from prophet_amd import reducer
from prophet_amd.compression import CastPlanCache, Compression, FP16Compressor
from prophet_amd.dtypes import DType
from prophet_amd.pushpull import ServerFrontend, Worker
from test_compress import RecordingServer

torch = pytest.importorskip("torch")

A, B, C, D = 0x10000, 0x80000, 0x100000, 0x180000   # never dereferenced
WIDE = (DType.FLOAT32, DType.FLOAT64, DType.BFLOAT16)


@pytest.fixture(scope="module")
def lib():
    return reducer.load_library()


def _segs(*triples):
    arr = (reducer.CastDesc * max(1, len(triples)))()
    for i, (w, h, n) in enumerate(triples):
        arr[i].wide, arr[i].half, arr[i].nelem = w, h, n
    return arr


def _create(lib, triples, dtype, nsegs=None):
    out = ctypes.c_void_p(0x1234)
    rc = lib.byteps_reduce_cast_plan_create(_segs(*triples), len(triples) if nsegs is None
                                            else nsegs, int(dtype), ctypes.byref(out))
    return rc, out


def test_argument_errors_without_a_gpu(lib):
    for dt in (DType.INT32, DType.UINT8, DType.INT64, DType.FLOAT16, 7, -1):
        rc, out = _create(lib, [(A, B, 64)], dt)
        assert rc == reducer.EDTYPE and not out.value
    assert b"data type" in lib.byteps_reduce_last_error()
    for dt in WIDE:
        assert _create(lib, [(A, B, 64), (None, D, 8)], dt)[0] == reducer.EARGS
        rc, out = _create(lib, [(A, B, 64), (C, None, 8)], dt)
        assert rc == reducer.EARGS and not out.value          # the out-pointer is cleared
        assert _create(lib, [(A, B, 64)], dt, nsegs=-1)[0] == reducer.EARGS
        assert lib.byteps_reduce_cast_plan_create(None, 2, int(dt),
                                                  ctypes.byref(ctypes.c_void_p())) == reducer.EARGS
        assert lib.byteps_reduce_cast_plan_create(_segs((A, B, 64)), 1, int(dt),
                                                  None) == reducer.EARGS
        assert _create(lib, [(A, B, ctypes.c_size_t(-1).value // 2)], dt)[0] == reducer.EARGS
    # launches: a null plan, and the divisor before anything else
    assert lib.byteps_reduce_cast_plan_compress(None, None) == reducer.EARGS
    assert lib.byteps_reduce_cast_plan_decompress(None, 1, None) == reducer.EARGS
    assert lib.byteps_reduce_cast_plan_destroy(None) == reducer.OK


def test_any_overlap_is_rejected(lib):
    f32 = DType.FLOAT32
    n = 100                                    # fp16: 200 bytes, f32: 400 bytes
    bad = [
        [(A, A, n)],                                        # a segment's two sides, same start
        [(A, A + 399, n)],                                  # half's first byte = wide's last
        [(A, B, n), (A + 396, D, n)],                       # wide / wide
        [(A, B, n), (C, B + 198, n)],                       # half / half
        [(A, B, n), (C, A + 399, n)],                       # another segment's half in a wide
        [(A, B, n), (B - 399, D, n)],                       # another segment's wide in a half
        [(A, B, n), (C, D, n), (A + 40, D + 0x1000, 10)],   # a range inside another
        [(A, B, n), (C, D, n), (A, B, n)],                  # the same segment twice
    ]
    for segs in bad:
        assert _create(lib, segs, f32)[0] == reducer.EARGS, segs
        assert b"overlap" in lib.byteps_reduce_last_error()
        assert _create(lib, segs[::-1], f32)[0] == reducer.EARGS, segs


def test_cast_plan_bounds_check_precedes_the_call(monkeypatch):
    red = reducer.GpuReducer()
    called = []
    monkeypatch.setattr(red.lib, "byteps_reduce_cast_plan_create",
                        lambda *a: called.append(a) or reducer.EARGS)
    half = torch.empty(100, dtype=torch.float16)
    wide = torch.empty(100, dtype=torch.float32)
    ok = (torch.empty(8, dtype=torch.float32), torch.empty(8, dtype=torch.float16), 8)
    for seg, dt in [((wide, half[:99], 100), DType.FLOAT32),      # fp16 side one element short
                    ((wide[:99], half, 100), DType.FLOAT32),      # wide side one element short
                    ((wide, half, 100), DType.FLOAT64),           # 400 bytes are 50 doubles
                    ((wide, half, -1), DType.FLOAT32)]:
        with pytest.raises(ValueError):
            red.cast_plan([ok, seg], dt)
    assert not called
    with pytest.raises(reducer.ReduceError):                      # in bounds: the library is asked
        red.cast_plan([ok, (wide, half, 100)], DType.FLOAT32)
    assert len(called) == 1


def _host_values(n, dt, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-26, 18, n))).astype(np.float64)
    x[:8] = [65504.0, -65520.0, 7e4, 1e-7, -3e-8, 0.0, -0.0, 6.1e-5][:min(8, n)]
    return torch.from_numpy(x).to(dt)


@pytest.mark.parametrize("divisor", [1, 3])
def test_many_into_on_host_tensors_equals_the_per_tensor_calls(divisor):
    dts = [torch.float32, torch.float64, torch.bfloat16, torch.float32]
    sizes = [1, 77, 1000, 4097]
    xs = [_host_values(n, dt, 5 + i) for i, (n, dt) in enumerate(zip(sizes, dts))]
    xs[1] = xs[1].numpy()                                         # numpy beside torch
    halves = [torch.empty(n, dtype=torch.float16) for n in sizes]
    halves[1] = halves[1].numpy()
    assert FP16Compressor.compress_many_into(halves, xs) is halves
    for h, x in zip(halves, xs):
        one = FP16Compressor.compress_into(np.empty_like(h) if isinstance(h, np.ndarray)
                                           else torch.empty_like(h), x)
        assert np.array_equal(np.asarray(h).view(np.uint16), np.asarray(one).view(np.uint16))
    outs = [np.empty_like(x) if isinstance(x, np.ndarray) else torch.empty_like(x) for x in xs]
    assert FP16Compressor.decompress_many_into(outs, halves, divisor) is outs
    for o, h in zip(outs, halves):
        one = FP16Compressor.decompress_into(np.empty_like(o) if isinstance(o, np.ndarray)
                                             else torch.empty_like(o), h, divisor)
        a, b = (torch.from_numpy(t) if isinstance(t, np.ndarray) else t for t in (o, one))
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # host tensors never build a plan
    cache = CastPlanCache()
    FP16Compressor.compress_many_into(halves, xs, plans=cache)
    assert len(cache) == 0 and cache.built == 0
    with pytest.raises(ValueError):
        FP16Compressor.decompress_many_into(outs, halves, 0)
    with pytest.raises(ValueError):
        FP16Compressor.compress_many_into(halves[:2], xs)


def _run_workers(n_workers, body):
    errors = []

    def run(rank):
        try:
            body(rank)
        except Exception as e:  # surfaced below
            errors.append(repr(e))
    ts = [threading.Thread(target=run, args=(r,)) for r in range(n_workers)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=30)
    assert not errors, errors


@pytest.mark.parametrize("average", [True, False])
def test_iteration_equals_per_tensor_push_pull(average):
    # Two workers: a two-operand fp16 sum does not depend on the arrival order
    # (no NaN), so the two runs below fold the same bits whichever worker the
    # stand-in server hears first.
    N = 2
    names = ["a", "b", "c", "d"]
    sizes = {"a": 2 * 500 + 77, "b": 333, "c": 1, "d": 1500}
    comp = {"a": Compression.fp16, "b": Compression.none, "c": Compression.fp16,
            "d": Compression.fp16}

    def grad(rank, name):
        rng = np.random.default_rng(10 * rank + len(name) + sizes[name])
        x = (rng.standard_normal(sizes[name]) * np.exp2(rng.integers(-20, 14, sizes[name])))
        if name == "b":                      # an fp16 tensor: travels as it is, also under
            return x.astype(np.float16)      # the stand-in server's fp16 fold
        x = x.astype(np.float64 if name == "d" else np.float32)
        x[:4] = [65519.0 - rank, 3e-8 * (rank + 1), -0.0, 7e4][:min(4, sizes[name])]
        return x

    def dtype_of(name):
        return {"b": DType.FLOAT16, "d": DType.FLOAT64}.get(name, DType.FLOAT32)

    results = {}
    for mode in ("iteration", "per tensor"):
        srv = RecordingServer(N)
        fe = ServerFrontend(srv, size=N)
        ws = [Worker(r, fe, partition_bytes=1000) for r in range(N)]
        held = {(r, n): grad(r, n) for r in range(N) for n in names}

        def body(rank, ws=ws, held=held, mode=mode):
            w = ws[rank]
            for n in names:
                w.declare(n)
            for n in names:
                w.init_tensor(n, np.zeros_like(held[(rank, n)]), dtype_of(n), compression=comp[n])
            if mode == "iteration":
                w.push_pull_iteration({n: held[(rank, n)] for n in names}, average=average)
            else:
                for n in reversed(names):
                    w.push_pull(n, held[(rank, n)], average=average)
            assert len(w._cast_plans) == 0          # host tensors: no plan
            w.close()
        _run_workers(N, body)
        results[mode] = held
    for key, got in results["iteration"].items():
        want = results["per tensor"][key]
        assert got.dtype == want.dtype
        assert not np.isnan(want.astype(np.float64)).any()
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), key
    # ... and something was actually summed and divided
    a0 = results["iteration"][(0, "a")]
    assert np.array_equal(a0, results["iteration"][(1, "a")]) and np.isinf(a0[3])


def test_iteration_average_needs_the_worker_count():
    srv = RecordingServer(1)
    w = Worker(0, ServerFrontend(srv, size=None), partition_bytes=1000)
    x = np.arange(10, dtype=np.float32)
    w.declare("g")
    w.init_tensor("g", x, DType.FLOAT32, compression=Compression.fp16)
    with pytest.raises(ValueError):
        w.push_pull_iteration({"g": x}, average=True)
