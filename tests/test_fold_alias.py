"""What "right" means when operands of a fold are one buffer, fixed on the
CPU before tests/test_fold_alias_gpu.py asks the GPU.

CpuReducer's loops are element-wise, so any exact alias is legal there, and
the in-place forms are the ones the reference uses.  On the pair table of
tests/fold_values.py (for fp16 also at the length with n % 8 == 5, whose last
rows lie in the scalar tail) the forms

    sum3(x, x, y)   sum3(y, x, y)   sum3(d, x, x)   sum3(x, x, x)   sum(x, x)

run with the host arrays aliased exactly like that, through the oracle port
and, where oracle/_ref is built, through the reference's compiled CpuReducer;
the two must agree (f32 / f64 rows whose operands are both NaN by class, as in
test_fold_values.assert_two_source_match).  The port called with aliased
arrays must also give what it gives for separate copies of the same values:
that is the expectation the GPU test uses.

fp16 is the dtype where the operand order of the 3-operand form shows: with
both operands NaN the body keeps src2's NaN, quieted, whichever of them dst
is, and the scalar tail turns every NaN into 0x7fff.
"""
import numpy as np
import pytest

import fold_values as fv
from oracle.oracle import PortReducer, RefReducer
from prophet_amd.dtypes import ALL_DTYPES, DType, REFERENCE_DTYPES
from test_fold_values import _is_nan, assert_two_source_match, ids, ref_only

FORMS = ("sum3_x_x_y", "sum3_y_x_y", "sum3_d_x_x", "sum3_x_x_x", "sum_x_x")


def run_form(red, form, dt, a, b):
    """`form` on fresh copies x of a and y of b, the host arrays aliased as the
    form's name says: (result, its first operand's values, its second's)."""
    x, y = a.copy(), b.copy()
    L = x.nbytes
    if form == "sum3_x_x_y":
        assert red.sum3(x, x, y, L, dt) == 0
        assert np.array_equal(y, b)
        return x, a, b
    if form == "sum3_y_x_y":
        assert red.sum3(y, x, y, L, dt) == 0
        assert np.array_equal(x, a)
        return y, a, b
    if form == "sum3_d_x_x":
        d = np.full_like(x, 0x5A)
        assert red.sum3(d, x, x, L, dt) == 0
        assert np.array_equal(x, a)
        return d, a, a
    if form == "sum3_x_x_x":
        assert red.sum3(x, x, x, L, dt) == 0
        return x, a, a
    assert form == "sum_x_x"
    assert red.sum(x, x, L, dt) == 0
    return x, a, a


def separate(red, form, dt, a, b):
    """The same values through separate buffers: what an element-wise reducer
    must also give for the aliased call."""
    s1, s2 = (a, b) if form in FORMS[:2] else (a, a)
    s1, s2 = s1.copy(), s2.copy()
    if form == "sum_x_x":
        assert red.sum(s1, s2, s1.nbytes, dt) == 0
        return s1
    d = np.zeros_like(s1)
    assert red.sum3(d, s1, s2, s1.nbytes, dt) == 0
    return d


def cuts(dt):
    a, b, _ = fv.pair_table(dt)
    out = [(a, b)]
    if dt == DType.FLOAT16:
        n = fv.fp16_tail_cut()
        out.append((np.ascontiguousarray(a[:n]), np.ascontiguousarray(b[:n])))
    return out


@ids(ALL_DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_port_aliased_equals_port_separate(dt, form):
    port = PortReducer(nthreads=4)
    for a, b in cuts(dt):
        got, _, _ = run_form(port, form, dt, a, b)
        assert np.array_equal(got, separate(port, form, dt, a, b)), (form, len(a))


@ref_only
@ids(REFERENCE_DTYPES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("threads", [1, 4])
def test_port_vs_reference_aliased(dt, form, threads):
    port, ref = PortReducer(nthreads=threads), RefReducer(nthreads=threads)
    for a, b in cuts(dt):
        got, s1, s2 = run_form(port, form, dt, a, b)
        exp, _, _ = run_form(ref, form, dt, a, b)
        assert_two_source_match(dt, s1, s2, got, exp,
                                f"{form} {DType(dt).name} n={len(a)} t={threads}")


@pytest.mark.parametrize("form", FORMS[:2])
def test_fp16_sum3_keeps_src2s_nan_whichever_operand_dst_is(form):
    """Both operands NaN: the body gives src2's NaN with the quiet bit set,
    in sum3(x, x, y) (dst is the other operand) and in sum3(y, x, y) (dst is
    src2 itself); the scalar tail gives 0x7fff."""
    dt = DType.FLOAT16
    port = PortReducer(nthreads=4)
    for a, b in cuts(dt):
        got, _, _ = run_form(port, form, dt, a, b)
        body = len(a) // 8 * 8
        both = _is_nan(dt, a) & _is_nan(dt, b)
        differ = both & ((a | 0x0200) != (b | 0x0200))
        assert int(differ[:body].sum()) >= 64          # the rows where the choice shows
        assert np.array_equal(got[:body][both[:body]], (b | 0x0200)[:body][both[:body]])
        if body < len(a):
            assert both[body:].any() and bool((got[body:][both[body:]] == 0x7FFF).all())


def test_doubling_and_self_sum_of_a_nan_quiet_it():
    """sum(x, x) and sum3(x, x, x): every NaN of x comes back quieted, in
    every float dtype (one operand read twice: no choice between payloads)."""
    port = PortReducer(nthreads=4)
    for dt, f in fv.FMT.items():
        a, b, _ = fv.pair_table(dt)
        n8 = len(a) // 8 * 8
        nan = _is_nan(dt, a)
        for form in FORMS[3:]:
            got, _, _ = run_form(port, form, dt, a, b)
            assert np.array_equal(got[:n8][nan[:n8]], (a | f.U.type(f.quiet))[:n8][nan[:n8]]), form
