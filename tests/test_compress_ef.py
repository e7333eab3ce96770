"""Error-feedback compression (Compression.fp16_ef / bf16_ef) without a GPU:
the host definition — c = g + r; w = wire(c); b = f32(w); r' = c - b where b is
finite, +0.0 elsewhere — on CPU torch tensors and numpy arrays, the scope
(float32 only), the plan cache's key, the Worker's residual through the host
server of tests/test_pushpull.py, and the argument checks of the two C calls,
all of which come before any HIP call."""
import ctypes

import numpy as np
import pytest

from prophet_amd import reducer
from prophet_amd.compression import (BF16Compressor, BF16EFCompressor, CastPlanCache,
                                     Compression, FP16Compressor, FP16EFCompressor)
from prophet_amd.dtypes import DType
from prophet_amd.pushpull import ServerFrontend, Worker
from test_pushpull import FakeServer

torch = pytest.importorskip("torch")

F16, BF16, F32 = int(DType.FLOAT16), int(DType.BFLOAT16), int(DType.FLOAT32)
WIRES = [(Compression.fp16_ef, Compression.fp16, torch.float16),
         (Compression.bf16_ef, Compression.bf16, torch.bfloat16)]
SPECIALS = np.array([np.inf, -np.inf, np.nan, 65519.99, 65520.0, -65519.99, -65520.0, 0.0, -0.0,
                     1e-45, -1e-40, 2.0 ** -25, 2.0 ** -24, 3.0e38, -3.4e38], np.float32)


def _data(n=1 << 14, seed=7):
    """f32 gradients over many decades, residuals of about half a wire ulp of
    the gradient in both signs, and the specials (0x7f7f8000: the first f32
    that bf16 rounds to inf)."""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(n) * np.exp2(rng.integers(-140, 126, n))).astype(np.float32)
    r = (g * np.exp2(-9.0) * rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.5, n))
    r = r.astype(np.float32)
    k = len(SPECIALS)
    g[:k] = SPECIALS
    r[:k] = 0
    g[k:2 * k] = SPECIALS
    r[k:2 * k] = np.float32(1e-3)
    g[2 * k] = np.array([0x7f7f8000], np.uint32).view(np.float32)[0]
    r[2 * k] = 0
    g[2 * k + 1], r[2 * k + 1] = np.float32(3.0e38), np.float32(3.0e38)      # g + r overflows f32
    return g, r


def _wire_bits(x):
    if isinstance(x, np.ndarray):
        return x.view(np.uint16).astype(np.int64)
    return x.view(torch.int16).numpy().view(np.uint16).astype(np.int64)


def _wire_f32(comp, x):
    """f32(w) of a host wire buffer."""
    return comp._host_wire(x).to(torch.float32)


@pytest.mark.parametrize("kind", ["torch", "numpy"])
@pytest.mark.parametrize("ef,plain,wire", WIRES)
def test_host_semantics(ef, plain, wire, kind):
    g, r0 = _data()
    wrap = torch.from_numpy if kind == "torch" else (lambda a: a)
    n = g.size
    # a zero residual: the bytes of compress_into — but for g = -0.0, which the
    # IEEE add turns into +0.0 (-0 + +0 = +0, round to nearest): the same value
    out, ref = ef.wire_like(wrap(g)), plain.wire_like(wrap(g))
    res = wrap(np.zeros(n, np.float32))
    assert ef.compress_ef_into(out, res, wrap(g.copy())) is out
    plain.compress_into(ref, wrap(g.copy()))
    neg0 = g.view(np.uint32) == 0x80000000
    assert neg0.sum() >= 2
    assert np.array_equal(_wire_bits(out)[~neg0], _wire_bits(ref)[~neg0])
    assert (_wire_bits(out)[neg0] == 0).all() and (_wire_bits(ref)[neg0] == 0x8000).all()
    assert (np.asarray(res).view(np.uint32) == 0)[neg0].all()
    # with a residual: f32(w) + r' == g + r exactly wherever f32(w) is finite,
    # r' has bits 0 wherever it is not
    res = wrap(r0.copy())
    ef.compress_ef_into(out, res, wrap(g.copy()))
    b = _wire_f32(ef, out)
    rn = torch.from_numpy(np.asarray(res))
    c = torch.from_numpy(g) + torch.from_numpy(r0)
    fin = torch.isfinite(b)
    assert fin.sum() > n // 2 and (~fin).sum() >= 6
    assert torch.equal(b.double()[fin] + rn.double()[fin], c.double()[fin])
    assert (rn.view(torch.int32)[~fin] == 0).all()
    assert torch.isfinite(rn).all()
    # the wire value is the plain compress of c
    assert np.array_equal(_wire_bits(out)[fin.numpy()],
                          _wire_bits(c.to(wire))[fin.numpy()])
    # the boundaries named by the wire format
    if wire == torch.float16:
        k = list(SPECIALS).index(np.float32(65519.99))
        assert np.isfinite(b[k].item()) and np.isinf(b[k + 1].item())
    else:
        assert np.isinf(b[2 * len(SPECIALS)].item())


@pytest.mark.parametrize("ef", [Compression.fp16_ef, Compression.bf16_ef])
def test_scope_is_float32(ef):
    assert ef.ERROR_FEEDBACK and not Compression.fp16.ERROR_FEEDBACK
    assert not Compression.none.ERROR_FEEDBACK
    assert issubclass(FP16EFCompressor, FP16Compressor)
    assert issubclass(BF16EFCompressor, BF16Compressor)
    for x in (torch.ones(4, dtype=torch.float64), torch.ones(4, dtype=torch.float16),
              torch.ones(4, dtype=torch.bfloat16), torch.ones(4, dtype=torch.int32),
              np.ones(4, np.float64), np.ones(4, np.float16), np.ones(4, np.int64)):
        assert not ef.compresses(x)
        y, ctx = ef.compress(x)
        assert y is x and ctx == x.dtype
        with pytest.raises(ValueError):
            ef.compress_ef_into(ef.wire_like(x), np.zeros(4, np.float32), x)
    for x in (torch.ones(4), np.ones(4, np.float32)):
        assert ef.compresses(x)
        # the stateless compress is the plain cast
        y, ctx = ef.compress(x)
        assert ctx == x.dtype and y.dtype != x.dtype
        back = ef.decompress(y, ctx)
        assert back.dtype == x.dtype and (np.asarray(back) == 1).all()
    with pytest.raises(ValueError):
        ef.compress_ef_into(ef.wire_like(torch.ones(4)), torch.zeros(4, dtype=torch.float64),
                            torch.ones(4))
    with pytest.raises(ValueError):
        ef.compress_many_ef_into([ef.wire_like(torch.ones(4))], [], [torch.ones(4)])


def test_many_on_the_host_is_one_by_one():
    g, r0 = _data(1000)
    for ef in (Compression.fp16_ef, Compression.bf16_ef):
        outs = [ef.wire_like(g[:300]), ef.wire_like(torch.from_numpy(g[300:]))]
        ress = [r0[:300].copy(), torch.from_numpy(r0[300:].copy())]
        plans = CastPlanCache(2)
        ef.compress_many_ef_into(outs, ress, [g[:300].copy(), torch.from_numpy(g[300:].copy())],
                                 plans=plans)
        assert len(plans) == 0 and plans.built == 0               # host tensors: no plans
        one, res = ef.wire_like(g), r0.copy()
        ef.compress_ef_into(one, res, g.copy())
        assert np.array_equal(np.concatenate([_wire_bits(o) for o in outs]), _wire_bits(one))
        assert np.array_equal(np.concatenate([np.asarray(x).view(np.uint32) for x in ress]),
                              res.view(np.uint32))
        back = [np.empty(300, np.float32), torch.empty(700)]
        ef.decompress_many_into(back, outs, 1, plans=plans, residuals=ress)
        want = _wire_f32(ef, one).numpy()
        got = np.concatenate([np.asarray(x) for x in back])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_plan_cache_key_carries_the_residual(monkeypatch):
    import prophet_amd.compression as comp

    class T:
        def __init__(self, p, n=8):
            self.p, self.n = p, n

        def data_ptr(self):
            return self.p

        def numel(self):
            return self.n

    class P:
        def close(self):
            pass

    made = []
    monkeypatch.setattr(comp, "_new_plan", lambda dt, pairs, wire=2: made.append(
        (dt, tuple(len(p) for p in pairs), wire)) or P())
    c = CastPlanCache(4)
    w, h, r, r2 = T(0x1000), T(0x2000), T(0x3000), T(0x4000)
    a = c.get(F32, [(w, h)])
    assert c.get(F32, [(w, h)]) is a and c.built == 1                # existing calls as before
    b = c.get(F32, [(w, h, r)])
    assert b is not a and c.built == 2                               # an EF plan is another plan
    assert c.get(F32, [(w, h, r)]) is b and c.built == 2
    assert c.get(F32, [(w, h, r2)]) is not b and c.built == 3        # a moved residual misses
    assert c.get(F32, [(w, h, r)], BF16) is not b and c.built == 4
    assert made[1] == (F32, (3,), 2)
    c.close()


class HalfServer(FakeServer):
    """tests/test_pushpull.py's host server under a 2-byte request dtype: with
    one worker its "sum" is the pushed bytes themselves."""

    def push(self, key, worker, data, dtype, nbytes=None):
        assert dtype in (DType.FLOAT16, DType.BFLOAT16)
        super().push(key, worker, np.asarray(data), DType.INT32, nbytes=nbytes)

    def pull(self, key, out, nbytes=None):
        super().pull(key, np.asarray(out), nbytes=nbytes)      # a CPU tensor's own memory


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_vanishing_gradient_is_delivered(kind):
    """One worker, fp16 wire, g = 1e-8 for 64 rounds: the plain compressor
    delivers exactly 0; with error feedback the delivered total is within one
    fp16 subnormal step (2^-24) of 64e-8 — the residual is bounded by half a
    step and the f32 add's own rounding is orders of magnitude smaller."""
    n, rounds = 8, 64
    wrap = (lambda a: a) if kind == "numpy" else torch.from_numpy
    totals = {}
    for name, comp in (("plain", Compression.fp16), ("ef", Compression.fp16_ef)):
        w = Worker(0, ServerFrontend(HalfServer(1), size=1))
        w.declare("g")
        ctx = w.init_tensor("g", wrap(np.zeros(n, np.float32)), DType.FLOAT32, compression=comp)
        assert ctx.dtype == DType.FLOAT16 and ctx.size == 2 * n
        total = np.zeros(n, np.float64)
        for _ in range(rounds):
            x = wrap(np.full(n, 1e-8, np.float32))
            w.push_pull("g", x)
            total += np.asarray(x).astype(np.float64)
        totals[name] = total
        if name == "plain":
            assert w.residual("g") is None
            w.reset_residual("g")                                  # nothing to do
        else:
            res = w.residual("g")
            assert res is ctx.residual and res.dtype == wrap(np.zeros(1, np.float32)).dtype
            assert np.isfinite(np.asarray(res)).all() and np.asarray(res).any()
            assert (np.abs(np.asarray(res)) <= 2.0 ** -25).all()
            w.reset_residual("g")
            assert (np.asarray(w.residual("g")).view(np.uint32) == 0).all()
            with pytest.raises(ValueError):
                w.broadcast("g", wrap(np.zeros(n, np.float32)), root_rank=0)
        w.close()
    assert (totals["plain"] == 0).all()
    assert (np.abs(totals["ef"] - rounds * 1e-8) <= 2.0 ** -24).all()
    assert (totals["ef"] > 0).all()


def test_worker_iteration_mixes_compressors_on_the_host():
    """push_pull_iteration over none / fp16 / bf16 / fp16_ef / bf16_ef contexts
    equals per-tensor push_pull, residuals included; the init push leaves the
    residual zero; f64 under an EF compressor passes through uncompressed."""
    n = 64
    g, r = _data(n * 5, seed=3)
    comps = {"a": Compression.none, "b": Compression.fp16, "c": Compression.bf16,
             "d": Compression.fp16_ef, "e": Compression.bf16_ef}

    def worker():
        w = Worker(0, ServerFrontend(HalfOrAnyServer(), size=1))
        for k in comps:
            w.declare(k)
        for i, (k, comp) in enumerate(comps.items()):
            ctx = w.init_tensor(k, g[i * n:(i + 1) * n].copy(), DType.FLOAT32, compression=comp)
            assert (ctx.residual is not None) == comp.ERROR_FEEDBACK
            if ctx.residual is not None:
                assert (ctx.residual.view(np.uint32) == 0).all()    # the init push: plain cast
        return w

    w1, w2 = worker(), worker()
    for step in range(3):
        with np.errstate(over="ignore"):
            x1 = {k: (g[i * n:(i + 1) * n] * np.float32(1 + step)).copy()
                  for i, k in enumerate(comps)}
        x2 = {k: v.copy() for k, v in x1.items()}
        for k in comps:
            w1.push_pull(k, x1[k])
        w2.push_pull_iteration(x2)
        for k in comps:
            assert np.array_equal(x1[k].view(np.uint32), x2[k].view(np.uint32)), (step, k)
        for k in ("d", "e"):
            assert np.array_equal(w1.residual(k).view(np.uint32), w2.residual(k).view(np.uint32))
            assert w1.residual(k).any()
    assert len(w2._cast_plans) == 0
    w = Worker(0, ServerFrontend(HalfOrAnyServer(), size=1))
    w.declare("f64")
    ctx = w.init_tensor("f64", np.zeros(8, np.float64), DType.FLOAT64,
                        compression=Compression.fp16_ef)
    assert ctx.compressor is None and ctx.residual is None and ctx.dtype == DType.FLOAT64


class HalfOrAnyServer:
    """One worker's host server: a pull returns the key's last push."""

    def __init__(self):
        self.store = {}

    def push(self, key, worker, data, dtype, nbytes=None):
        self.store[key] = np.asarray(data).view(np.uint8).copy()

    def pull(self, key, out, nbytes=None):
        np.asarray(out).view(np.uint8)[:] = self.store[key]


# ------------------------------------------------------------- C ABI checks --
A, B, C, D, E, F = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000


@pytest.fixture(scope="module")
def lib():
    return reducer.load_library()


def test_compress_ef_argument_errors_without_a_gpu(lib):
    ef = lib.byteps_reduce_compress_ef
    for dt in (DType.FLOAT64, DType.FLOAT16, DType.BFLOAT16, DType.INT32, DType.UINT8, 7, -1):
        for wire in (F16, BF16):
            assert ef(A, B, C, 64, int(dt), wire, None) == reducer.EDTYPE, (dt, wire)
            assert b"data type" in lib.byteps_reduce_last_error()
    for wire in (F32, int(DType.FLOAT64), int(DType.INT32), 7, -1):
        assert ef(A, B, C, 64, F32, wire, None) == reducer.EDTYPE, wire
    for wire in (F16, BF16):
        assert ef(None, B, C, 64, F32, wire, None) == reducer.EARGS
        assert ef(A, None, C, 64, F32, wire, None) == reducer.EARGS
        assert ef(A, B, None, 64, F32, wire, None) == reducer.EARGS
        assert b"null" in lib.byteps_reduce_last_error()
        # the three ranges pairwise: dst 128 bytes, resid and src 256
        assert ef(A, A, C, 64, F32, wire, None) == reducer.EARGS            # dst / resid
        assert ef(A, B, A + 127, 64, F32, wire, None) == reducer.EARGS      # dst / src
        assert ef(A, B, B + 255, 64, F32, wire, None) == reducer.EARGS      # resid / src
        assert ef(A, B, B, 64, F32, wire, None) == reducer.EARGS
        assert ef(B + 255, B, C, 64, F32, wire, None) == reducer.EARGS
        assert b"overlap" in lib.byteps_reduce_last_error()
        assert ef(None, None, None, 0, F32, wire, None) == reducer.OK       # nothing to do
        assert ef(A, B, C, ctypes.c_size_t(-1).value // 2, F32, wire, None) == reducer.EARGS
    assert lib.byteps_reduce_version() == 5


def _segs(*quads):
    arr = (reducer.CastEfDesc * max(1, len(quads)))()
    for i, (w, h, r, n) in enumerate(quads):
        arr[i].wide, arr[i].half, arr[i].resid, arr[i].nelem = w, h, r, n
    return arr


def test_ef_plan_argument_errors_without_a_gpu(lib):
    def create(quads, dt, wire, nsegs=None):
        out = ctypes.c_void_p(0x1234)
        rc = lib.byteps_reduce_cast_plan_create_ef(
            _segs(*quads), len(quads) if nsegs is None else nsegs, int(dt), int(wire),
            ctypes.byref(out))
        return rc, out

    for dt, wire in [(DType.FLOAT64, F16), (DType.BFLOAT16, F16), (DType.FLOAT16, BF16),
                     (DType.INT32, BF16), (7, F16), (F32, F32), (F32, -1)]:
        rc, out = create([(A, B, C, 64)], dt, wire)
        assert rc == reducer.EDTYPE and not out.value, (dt, wire)
        assert b"data type" in lib.byteps_reduce_last_error()
    for wire in (F16, BF16):
        rc, out = create([(A, B, C, 64), (D, E, None, 8)], F32, wire)       # null residual
        assert rc == reducer.EARGS and not out.value
        assert create([(A, B, C, 64), (None, E, F, 8)], F32, wire)[0] == reducer.EARGS
        assert create([(A, B, C, 64)], F32, wire, nsegs=-1)[0] == reducer.EARGS
        assert lib.byteps_reduce_cast_plan_create_ef(
            None, 2, F32, wire, ctypes.byref(ctypes.c_void_p())) == reducer.EARGS
        assert lib.byteps_reduce_cast_plan_create_ef(_segs((A, B, C, 64)), 1, F32, wire,
                                                     None) == reducer.EARGS
        # overlap between any two of the 3 * nsegs ranges
        for bad in ([(A, B, A, 100)], [(A, B, B + 199, 100)],
                    [(A, B, C, 100), (D, E, C + 399, 100)], [(A, B, C, 100), (D, C + 4, F, 100)],
                    [(A, B, C, 100), (C, E, F, 100)], [(A, B, C, 100), (D, E, A + 396, 100)]):
            assert create(bad, F32, wire)[0] == reducer.EARGS, bad
            assert b"overlap" in lib.byteps_reduce_last_error()


def test_reducer_bounds_checks_cover_the_residual(monkeypatch):
    red = reducer.GpuReducer()
    called = []
    for name in ("byteps_reduce_compress_ef", "byteps_reduce_cast_plan_create_ef"):
        monkeypatch.setattr(red.lib, name,
                            lambda *a, name=name: called.append(name) or reducer.EARGS)
    wire = torch.empty(100, dtype=torch.float16)
    wide = torch.empty(100, dtype=torch.float32)
    short = torch.empty(99, dtype=torch.float32)
    with pytest.raises(ValueError):
        red.compress_ef(wire, short, wide, 100, DType.FLOAT32, DType.FLOAT16)   # residual short
    with pytest.raises(ValueError):
        red.compress_ef(wire[:99], wide.clone(), wide, 100, DType.FLOAT32, DType.FLOAT16)
    with pytest.raises(ValueError):
        red.cast_plan([(wide, wire, 100, short)], DType.FLOAT32)
    with pytest.raises(ValueError):                                 # residuals: all or none
        red.cast_plan([(wide, wire, 100, wide.clone()), (wide, wire, 100)], DType.FLOAT32)
    assert not called
    with pytest.raises(reducer.ReduceError):
        red.compress_ef(wire, wide.clone(), wide, 100, DType.FLOAT32, DType.FLOAT16)
    with pytest.raises(reducer.ReduceError):
        red.cast_plan([(wide, wire, 100, wide.clone())], DType.FLOAT32, DType.BFLOAT16)
    assert called == ["byteps_reduce_compress_ef", "byteps_reduce_cast_plan_create_ef"]


def test_ops_are_registered_and_mutate_both():
    from prophet_amd import torch_ops
    for name in ("compress_fp16_ef_out", "compress_bf16_ef_out"):
        assert name in torch_ops.OPS
        s = str(getattr(torch.ops.bpsr, name).default._schema)
        assert "Tensor(a0!) dst" in s and "Tensor(a1!) resid" in s and "Tensor src" in s
        with pytest.raises(NotImplementedError):                   # no CPU kernel
            getattr(torch.ops.bpsr, name)(torch.empty(4, dtype=torch.float16), torch.zeros(4),
                                          torch.ones(4))
