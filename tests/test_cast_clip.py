"""Clip by global norm and unscale inside the decompress, the
parts that need no GPU: the pinned definition ``compression.clip_record``
against hand-computed values, the host-tensor and numpy path of
``decompress_many_into(clip_norm=)`` and ``measure_many_with`` against the
definition, argument validation in Python, and the three entry points'
declarations and exports."""
import os
import re
import subprocess

import numpy as np
import pytest

from prophet_amd import reducer
from prophet_amd.compression import (ClipValues, Compression, clip_record, decompress_stats)

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["byteps_reduce_cast_plan_measure", "byteps_reduce_clip_record",
       "byteps_reduce_cast_plan_decompress_scaled"]
INF, NAN = float("inf"), float("nan")


# --------------------------------------------------------------- definition --
def test_clip_record_by_hand():
    # 3-4-5: sumsq 25, norm 5, clipped to 2.5 with eps 0: c = 0.5
    r = clip_record(np.array([[9.0, 0.0], [16.0, 1.0]]), 2.5, 0.0)
    assert isinstance(r, ClipValues)
    assert (r.sumsq, r.nonfinite, r.norm) == (25.0, 1.0, 5.0) and r.found_inf == 1.0
    assert r.coef.dtype == np.float32 and r.mult.dtype == np.float32
    assert (float(r.coef), float(r.mult)) == (0.5, 0.5)
    # the norm is the UNSCALED gradients': sqrt(sumsq) * inv_scale; mult carries both
    r = clip_record(np.array([9.0, 0.0, 16.0, 0.0]), 2.5, 0.0, 0.5)
    assert (r.norm, float(r.coef), float(r.mult)) == (2.5, 1.0, 0.5)
    r = clip_record(np.array([[9.0, 0.0], [16.0, 0.0]]), 1.25, 0.0, 0.5)
    assert (r.norm, float(r.coef), float(r.mult)) == (2.5, 0.5, 0.25)
    # eps enters the quotient: 1 / (5 + 3) in f64, then one f32 rounding
    r = clip_record(np.array([[25.0, 0.0]]), 1.0, 3.0)
    assert float(r.coef) == 0.125
    r = clip_record(np.array([[2.0, 0.0]]), 1.0)
    assert r.coef == np.float32(1.0 / (np.sqrt(2.0) + 1e-6))
    # below the bound: coef is 1 exactly, mult is inv_scale bit for bit
    inv = np.float32(1.0 / 3.0)
    r = clip_record(np.array([[1e-4, 0.0]]), 1.0, 1e-6, inv)
    assert float(r.coef) == 1.0 and r.mult == inv
    # no rows, all-zero rows (eps 0 included): sumsq 0, coef 1
    for rows in (np.empty((0, 2)), np.zeros((4, 2)), torch.zeros((2, 2), dtype=torch.float64)):
        for eps in (1e-6, 0.0):
            r = clip_record(rows, 1.0, eps, 2.0 ** -16)
            assert (r.sumsq, r.nonfinite, r.norm) == (0.0, 0.0, 0.0)
            assert (float(r.coef), float(r.mult)) == (1.0, 2.0 ** -16)
    # non-finite values are counted, they do not poison the norm
    r = clip_record(np.array([[4.0, 7.0], [0.0, 2.0 ** 40]]), 1.0, 0.0)
    assert (r.nonfinite, r.norm, float(r.coef)) == (7.0 + 2.0 ** 40, 2.0, 0.5)
    for bad in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError, match="max_norm"):
            clip_record(np.zeros((1, 2)), bad)
    for bad in (-1e-9, NAN):
        with pytest.raises(ValueError, match="eps"):
            clip_record(np.zeros((1, 2)), 1.0, bad)


# ---------------------------------------------------------------- host path --
def _scaled(plain, m):
    """The scaled decompress's rounding on the host."""
    m32 = torch.tensor(float(m), dtype=torch.float32)
    if plain.dtype == torch.float64:
        return plain * m32.double()
    if plain.dtype == torch.float32:
        return plain * m32
    return (plain.float() * m32).to(plain.dtype)


@pytest.mark.parametrize("name", ["fp16", "bf16", "fp16_ef", "bf16_sr"])
@pytest.mark.parametrize("kind", ["torch", "numpy"])
def test_host_path_against_the_definition(name, kind):
    comp = getattr(Compression, name)
    wire = comp.wire_torch_dtype()
    g = torch.Generator().manual_seed(3)
    sizes = [300, 0, 2048 + 9, 77]
    if kind == "numpy" or name not in ("fp16", "bf16"):
        dts = [torch.float32, torch.float32, torch.float64, torch.float32]
    else:
        dts = [torch.float32, torch.float64, torch.float32,
               torch.bfloat16 if name == "fp16" else torch.float16]
    ws = []
    for n in sizes:
        x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-4, 4, (n,), generator=g))
        if n > 5:
            x[1], x[5] = INF, NAN
        ws.append(x.to(wire))
    plain = [torch.empty(n, dtype=dt) for n, dt in zip(sizes, dts)]
    comp.decompress_many_into(plain, ws, 8)
    want_rows = np.array([decompress_stats(p) for p in plain], dtype=np.float64)

    def fresh():
        outs = [torch.full((n,), -77.0, dtype=dt) for n, dt in zip(sizes, dts)]
        if kind == "numpy":
            return [o.numpy() for o in outs], \
                [w.view(torch.int16).numpy().view(np.uint16) if name.startswith("bf16")
                 else w.numpy() for w in ws]
        return outs, ws

    # measure_many_with: the rows, and nothing written
    outs, wires = fresh()
    st = np.full((4, 2), NAN) if kind == "numpy" else torch.full((4, 2), NAN, dtype=torch.float64)
    assert comp.measure_many_with(outs, wires, None, 8, None, st) is st
    assert np.array_equal(np.asarray(st), want_rows)
    assert all(bool((torch.as_tensor(o) == -77.0).all()) for o in outs)
    # the clip: pre-clip rows into stats, the record is the definition's, the
    # outputs are mult times the plain decompress under the rounding rule
    total = float(np.sqrt(want_rows[:, 0].sum())) * 2.0 ** -7
    for clip, unscale in ((total / 2, 2.0 ** -7), (total * 2, 2.0 ** -7), (total / 2, None),
                          (total / 2, torch.tensor([2.0 ** -7]))):
        outs, wires = fresh()
        st = np.full((4, 2), NAN) if kind == "numpy" else \
            torch.full((4, 2), NAN, dtype=torch.float64)
        rec = comp.decompress_many_into(outs, wires, 8, stats=st, clip_norm=clip, unscale=unscale)
        assert isinstance(rec, ClipValues) and np.array_equal(np.asarray(st), want_rows)
        inv = None if unscale is None else 2.0 ** -7
        want = clip_record(want_rows, clip, 1e-6, inv)
        assert (rec.sumsq, rec.nonfinite, rec.norm, rec.coef, rec.mult) == \
            (want.sumsq, want.nonfinite, want.norm, want.coef, want.mult)
        assert rec.nonfinite == 6.0 and np.isfinite(rec.norm)
        if clip > total and unscale is not None:
            assert float(rec.coef) == 1.0 and float(rec.mult) == 2.0 ** -7
        for o, p in zip(outs, plain):
            got, ref = torch.as_tensor(o), _scaled(p, rec.mult)
            nan = torch.isnan(ref)
            assert torch.equal(torch.isnan(got), nan)
            assert torch.equal(got[~nan], ref[~nan])
            assert torch.equal(torch.isinf(got), torch.isinf(p))          # inf stays inf


def test_argument_validation():
    comp = Compression.fp16
    w = torch.ones(4, dtype=torch.float16)
    out = torch.empty(4)
    for bad in (0.0, -2.0, INF, NAN):
        with pytest.raises(ValueError, match="clip_norm"):
            comp.decompress_many_into([out], [w], 1, clip_norm=bad)
    with pytest.raises(ValueError, match="clip_eps"):
        comp.decompress_many_into([out], [w], 1, clip_norm=1.0, clip_eps=-1.0)
    with pytest.raises(ValueError, match="unscale goes with clip_norm"):
        comp.decompress_many_into([out], [w], 1, unscale=0.5)
    for c in (Compression.fp16_ef, Compression.bf16_sr):
        with pytest.raises(ValueError, match="unscale goes with clip_norm"):
            c.decompress_many_into([out], [w.to(c.wire_torch_dtype())], 1, unscale=0.5)
    with pytest.raises(ValueError, match="shape"):
        comp.decompress_many_into([out], [w], 1, clip_norm=1.0, stats=np.empty((2, 2)))
    with pytest.raises(ValueError, match="as many"):
        comp.decompress_many_into([out, out], [w], 1, clip_norm=1.0)
    with pytest.raises(ValueError, match="needs stats"):
        comp.measure_many_with([out], [w], None, 1, None, None)
    with pytest.raises(ValueError, match="divisor"):
        comp.measure_many_with([out], [w], None, 0, None, np.empty((1, 2)))
    from prophet_amd.compression import _cast_many
    with pytest.raises(ValueError, match="scale is a decompress without stats"):
        _cast_many(comp, [(out, w)], False, 1, None, stats=np.empty((1, 2)), scale=0.5)
    with pytest.raises(ValueError, match="measure is a decompress with stats"):
        _cast_many(comp, [(out, w)], False, 1, None, measure=True)
    # the library refuses before any device call
    lib = reducer.load_library()
    assert lib.byteps_reduce_cast_plan_measure(None, 1, None, None) == reducer.EARGS
    assert b"null plan" in lib.byteps_reduce_last_error()
    assert lib.byteps_reduce_cast_plan_decompress_scaled(None, 1, None, None) == reducer.EARGS
    assert b"null plan" in lib.byteps_reduce_last_error()
    assert lib.byteps_reduce_clip_record(None, 1, 1.0, 1e-6, None, None, None) == reducer.EARGS
    assert b"null rows" in lib.byteps_reduce_last_error()
    assert lib.byteps_reduce_clip_record(None, 0, 1.0, 1e-6, None, None, None) == reducer.EARGS
    assert b"null clip record" in lib.byteps_reduce_last_error()
    assert lib.byteps_reduce_clip_record(None, -1, 1.0, 1e-6, None, 8, None) == reducer.EARGS
    assert lib.byteps_reduce_clip_record(None, 0, 1.0, 1e-6, None, 12, None) == reducer.EARGS
    assert b"aligned" in lib.byteps_reduce_last_error()
    for bad in (0.0, -1.0, INF, NAN):
        assert lib.byteps_reduce_clip_record(None, 0, bad, 1e-6, None, 8, None) == reducer.EARGS
        assert b"max_norm" in lib.byteps_reduce_last_error()
    for bad in (-1e-9, NAN):
        assert lib.byteps_reduce_clip_record(None, 0, 1.0, bad, None, 8, None) == reducer.EARGS
        assert b"eps" in lib.byteps_reduce_last_error()


def test_worker_keywords_are_validated_before_anything_is_pushed():
    from prophet_amd.pushpull import GradClip, Worker

    class Frontend:
        size = 2

        def push(self, *a):
            raise AssertionError("nothing is pushed")

    w = Worker(0, Frontend())
    assert w.grad_clip is None
    with pytest.raises(ValueError, match="unscale goes with clip_norm"):
        w.push_pull_iteration({}, unscale=0.5)
    for bad in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError, match="clip_norm"):
            w.push_pull_iteration({}, clip_norm=bad)
    with pytest.raises(ValueError, match="clip_eps"):
        w.push_pull_iteration({}, clip_norm=1.0, clip_eps=-1.0)
    assert GradClip.__doc__ and "found_inf" in GradClip.__doc__


# ---------------------------------------------------------------------- ABI --
def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "bpsr", "reduce.h")).read()
    for sym in NEW:
        assert re.search(r"\bint " + sym + r"\(", hdr), sym
        assert sym in reducer.EXPORTS
    assert re.search(r"typedef struct byteps_clip_record \{\s*double sumsq;\s*double nonfinite;"
                     r"\s*double norm;\s*float coef;\s*float mult;\s*\} byteps_clip_record;", hdr)
    assert "#define BYTEPS_REDUCE_ABI_VERSION 5" in hdr          # additive
    out = subprocess.run(["nm", "-D", "--defined-only", reducer.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW) <= exported
    lib = reducer.load_library()
    assert lib.byteps_reduce_version() == 5
