"""The probe inputs of tests/order_probe.py really are sensitive to the fold's
order: conditions on the inputs, checked against the oracle alone, for every
(dtype, workers, key shape) that tests/test_server_order_gpu.py and
tests/test_parity_probe_gpu.py use — so that a pass on the GPU means the
kernels folded in the recorded order, NaN replay included.  No GPU."""
import numpy as np
import pytest

import order_probe as op
from oracle.oracle import PortReducer
from prophet_amd.dtypes import DType

SERVER = sorted(set(op.DEVICE_NARROW + op.DEVICE_WIDE + op.LAUNCH + op.COPIED),
                key=lambda c: (int(c[1]), c[0]))
WIDE = [c for c in SERVER if c[0] > 8]
DIRECT = [(n, dt) for dt in op.DIRECT_DTYPES for n in op.DIRECT_N]
RAGGED, TILE_PLUS_1 = 3, 2          # indices into op.server_keys


@pytest.fixture(scope="module")
def port():
    return PortReducer(nthreads=1)


def ident(n):
    return list(range(n))


@pytest.mark.parametrize("case", SERVER, ids=op.case_id)
def test_adjacent_swaps_show_in_every_tile_region(port, case):
    """For each of the three orders (and each round's data), exchanging any
    two adjacent arrivals changes the oracle's bytes in at least one probe
    element of each full-tile region of the ragged key, of its partial tile,
    and of the one-tile key."""
    N, dt = case
    for rnd in range(1, op.ROUNDS + 1):
        for j, names in ((RAGGED, ("first_tile", "last_full_tile", "partial_tile")),
                         (TILE_PLUS_1, ("tile",))):
            ins, kind = op.server_inputs(dt, N, rnd, j)
            reg = op.server_keys(dt)[j][1]
            for order in op.orders(N):
                base = op.fold(port, dt, ins, order)
                for i in range(N - 1):
                    d = op.changed(dt, base, op.fold(port, dt, ins, op.swapped(order, i)))
                    d &= kind >= 0
                    for name in names:
                        lo, hi = reg[name]
                        assert d[lo:hi].any(), (rnd, j, order, i, name)


@pytest.mark.parametrize("case", SERVER, ids=op.case_id)
def test_first_swap_shows_in_the_vector_tail(port, case):
    """Exchanging the first two arrivals changes at least one of the elements
    behind the last whole vector (fp32: the last 3, fp64: the last one, bf16:
    the last 5).  fp16 has none at this shape: its 5 ragged elements are all
    scalar tail (next test), where no NaN names a worker."""
    N, dt = case
    n, _ = op.server_keys(dt)[RAGGED]
    vt = op.vector_tail(dt, n)
    if DType(dt) == DType.FLOAT16:
        assert len(vt) == 0 and len(op.f16_scalar_tail(dt, n)) == 5
        return
    assert len(vt) == op.ragged_tail(dt)
    for rnd in range(1, op.ROUNDS + 1):
        ins, kind = op.server_inputs(dt, N, rnd, RAGGED)
        assert (kind[vt.start:vt.stop] >= 0).all()
        for order in op.orders(N):
            d = op.changed(dt, op.fold(port, dt, ins, order),
                           op.fold(port, dt, ins, op.swapped(order, 0)))
            assert d[vt.start:vt.stop].any(), (rnd, order)


def _body_rule(port, ins, elems, order):
    """The fp16 body rule's result for elements `elems`: the same columns
    folded at the start of a 16-element array (floor(16 / 8) * 8 = 16: no
    scalar tail)."""
    cols = []
    for x in ins:
        c = np.zeros(16, np.uint16)
        c[:len(elems)] = x.view(np.uint16)[elems.start:elems.stop]
        cols.append(c.view(np.uint8))
    return op.fold(port, DType.FLOAT16, cols, order).view(np.uint16)[:len(elems)]


@pytest.mark.parametrize("case", [c for c in SERVER if c[1] == DType.FLOAT16], ids=op.case_id)
def test_f16_scalar_tail_holds_a_nan_the_body_rule_would_keep(port, case):
    """fp16: at least one scalar-tail element's result is 0x7fff where the
    body rule would give another NaN (a payload, or the default 0xfe00)."""
    N, dt = case
    for j in (1, TILE_PLUS_1, RAGGED):           # 7 elements: all of them scalar tail
        n = op.server_keys(dt)[j][0]
        st = op.f16_scalar_tail(dt, n)
        assert len(st) > 0
        for rnd in range(1, op.ROUNDS + 1):
            ins, _ = op.server_inputs(dt, N, rnd, j)
            order = op.round_order(N, rnd, j)
            got = op.fold(port, dt, ins, order).view(np.uint16)[st.start:st.stop]
            body = _body_rule(port, ins, st, order)
            assert ((got == 0x7FFF) & (body != 0x7FFF)).any(), (j, rnd)


@pytest.mark.parametrize("case", SERVER, ids=op.case_id)
def test_slot_order_changes_nan_results(port, case):
    """The replay's share: folding in slot order 0..N-1 instead of a test
    order changes probe elements whose expected result is a NaN — in each tile
    region of the ragged key.  (N = 2's third order is the identity itself:
    nothing to tell apart there.)"""
    N, dt = case
    reg = op.server_keys(dt)[RAGGED][1]
    for rnd in range(1, op.ROUNDS + 1):
        ins, kind = op.server_inputs(dt, N, rnd, RAGGED)
        slot = op.fold(port, dt, ins, ident(N))
        for order in op.orders(N):
            if order == ident(N):
                continue
            want = op.fold(port, dt, ins, order)
            d = op.changed(dt, want, slot) & (kind >= 0) & op.is_nan(dt, want)
            for name in ("first_tile", "last_full_tile", "partial_tile"):
                lo, hi = reg[name]
                assert d[lo:hi].any(), (rnd, order, name)


@pytest.mark.parametrize("case", WIDE, ids=op.case_id)
def test_second_release_word_changes_results(port, case):
    """The second release word's share (positions 8..15 of the order).  With
    12 and 16 workers, replacing those positions by their identity values
    changes NaN-result probe elements for every order.  With 9 workers the
    second word holds the last arrival alone, which names no NaN (the first
    NaN that came decides) — there the finite lanes and maxfin carry it: the
    bytes change for every order whose last arrival is not worker 8."""
    N, dt = case
    for rnd in range(1, op.ROUNDS + 1):
        ins, kind = op.server_inputs(dt, N, rnd, RAGGED)
        for order in op.orders(N):
            reset = op.second_word_reset(order)
            if reset == order:
                assert N == 9
                continue
            want = op.fold(port, dt, ins, order)
            d = op.changed(dt, want, op.fold(port, dt, ins, reset))
            if N >= 12:
                d &= (kind >= 0) & op.is_nan(dt, want)
            assert d.any(), (rnd, order)


def _server_case_mismatches(port, N, dt, wrong):
    """Per (round, key index): how many elements the expectation of
    test_server_order_gpu (the oracle in round_order) differs in from the
    oracle folding in wrong(order)."""
    out = {}
    for rnd in range(1, op.ROUNDS + 1):
        for j in range(4):
            ins, _ = op.server_inputs(dt, N, rnd, j)
            order = op.round_order(N, rnd, j)
            out[(rnd, j)] = int(op.changed(dt, op.fold(port, dt, ins, order),
                                           op.fold(port, dt, ins, wrong(order))).sum()), order
    return out


@pytest.mark.parametrize("case", SERVER, ids=op.case_id)
def test_the_server_tests_can_fail(port, case):
    """The GPU expectations re-run here with the oracle folding in a wrong
    order: slot order mismatches in every key of every round whose order is
    not the identity (the 1-element key included: its `all` probe names the
    first arrival — but for fp16, whose 1- and 7-element keys are scalar tail
    alone, where every NaN is 0x7fff: the tile keys only); with more than 8
    workers, positions 8.. reset mismatch in the tile keys whenever they
    differ from the order."""
    N, dt = case
    for (rnd, j), (bad, order) in _server_case_mismatches(port, N, dt,
                                                          lambda o: ident(N)).items():
        if order != ident(N) and (j >= TILE_PLUS_1 or DType(dt) != DType.FLOAT16):
            assert bad > 0, ("slot order", rnd, j)
    if N > 8:
        hit = 0
        for (rnd, j), (bad, order) in _server_case_mismatches(port, N, dt,
                                                              op.second_word_reset).items():
            if j >= TILE_PLUS_1 and op.second_word_reset(order) != order:
                assert bad > 0, ("second word", rnd, j)
                hit += 1
        assert hit >= 4


def test_big_key_probes(port):
    """The 16 MiB key of the real-tile-size case (8 workers, fp32, reversed
    order): in the first tile, the last full tile and the tail, every adjacent
    swap changes probe elements (the tail: the first swap), and slot order
    changes NaN-result probe elements.  fp32 folds element by element, so the
    regions are folded on their own."""
    dt, N = DType.FLOAT32, 8
    ins, kind = op.big_inputs(N)
    n, reg = op.big_key()
    assert int((kind >= 0).sum()) == sum(len(range(lo, hi, 3 if hi - lo >= op.DENSE_BELOW else 1))
                                         for lo, hi in reg.values())
    order = op.orders(N)[0]
    for name, (lo, hi) in reg.items():
        part = [np.ascontiguousarray(x[4 * lo:4 * hi]) for x in ins]
        k = kind[lo:hi]
        want = op.fold(port, dt, part, order)
        for i in range(N - 1 if name != "tail" else 1):
            d = op.changed(dt, want, op.fold(port, dt, part, op.swapped(order, i)))
            assert (d & (k >= 0)).any(), (name, i)
        d = op.changed(dt, want, op.fold(port, dt, part, ident(N)))
        assert (d & (k >= 0) & op.is_nan(dt, want)).any(), name


@pytest.mark.parametrize("case", DIRECT, ids=op.case_id)
def test_direct_calls_adjacent_source_swaps_show(port, case):
    """The direct calls fold in the caller's source order: exchanging any two
    adjacent sources changes NaN-result probe elements (with 40 sources the
    fp64 shape is too short for every pair: the list's head — every clash,
    the pairs up to some distance — still tells every adjacent swap), the
    first swap changes the vector tail, and fp16's scalar tail holds a 0x7fff
    the body rule would not give.  The same at the co-aligned byte offsets'
    heads (fp16 and fp32, 8 and 9 sources), where the head, the elements
    behind the last vector and the scalar tail all hold NaN probes (fp16's
    head of 1 leaves no body element behind the last vector:
    order_probe.ragged_key)."""
    n_src, dt = case
    es = np.dtype(op.bits_type(dt)).itemsize
    heads = [0]
    if n_src in (8, 9):
        heads += [(16 - off) // es for off in op.DIRECT_OFFSETS.get(DType(dt), [])]
    for head in heads:
        ins, kind, n, reg = op.direct_inputs(dt, n_src, head)
        want = op.fold(port, dt, ins, ident(n_src))
        nan = op.is_nan(dt, want)
        for i in range(n_src - 1):
            d = op.changed(dt, want, op.fold(port, dt, ins, op.swapped(ident(n_src), i)))
            assert (d & (kind >= 0) & nan).any(), (head, i)
            if i == 0:
                vt = op.vector_tail(dt, n, head)
                if len(vt):
                    assert d[vt.start:vt.stop].any(), head
                if head:
                    assert d[:head].any(), head
        st = op.f16_scalar_tail(dt, n)
        if DType(dt) == DType.FLOAT16:
            assert len(st) == (3 if head else 5)
            got = want.view(np.uint16)[st.start:st.stop]
            assert ((got == 0x7FFF) & (_body_rule(port, ins, st, ident(n_src)) != 0x7FFF)).any()
            if head:
                assert nan[:head].any()
                vt = op.vector_tail(dt, n, head)
                if head == 1:       # the scalar tail begins inside the last vector
                    assert len(vt) == 0 and reg["tail"][0] == st.start + 1
                else:
                    assert len(vt) > 0 and nan[vt.start:vt.stop].any()


@pytest.mark.parametrize("dt", op.DIRECT_DTYPES, ids=lambda d: DType(d).name)
def test_element_path_adjacent_source_swaps_show(port, dt):
    """The bucket that is element work only (4 sources): every adjacent swap
    changes NaN-result probe elements; fp16's 7 scalar-tail elements hold a
    0x7fff the body rule would not give."""
    ins, kind, n, _ = op.element_path_inputs(dt)
    want = op.fold(port, dt, ins, ident(4))
    for i in range(3):
        d = op.changed(dt, want, op.fold(port, dt, ins, op.swapped(ident(4), i)))
        assert (d & (kind >= 0) & op.is_nan(dt, want)).any(), i
    if DType(dt) == DType.FLOAT16:
        st = op.f16_scalar_tail(dt, n)
        got = want.view(np.uint16)[st.start:st.stop]
        assert ((got == 0x7FFF) & (_body_rule(port, ins, st, ident(4)) != 0x7FFF)).any()


def test_orders_are_what_they_say():
    for n in (2, 3, 4, 8, 9, 12, 16):
        rev, rot, mix = op.orders(n)
        for o in (rev, rot, mix):
            assert sorted(o) == ident(n)
        assert rev == ident(n)[::-1]
        assert all(rot[i] != i for i in range(n))
        if n >= 4:
            assert all(abs(mix[i] - mix[i + 1]) != 1 for i in range(n - 1))
    assert {tuple(op.round_order(8, 1, j)) for j in range(3)} == {tuple(o) for o in op.orders(8)}


def test_probe_values():
    """The probe elements hold what the module says (8 workers, fp32, one
    dense region and one at every third element)."""
    dt, N = DType.FLOAT32, 8
    ins, kind = op.inputs(dt, 400, N, 1, [(0, 20), (40, 400)])
    K = op.kinds(N)
    assert len(K) == 4 + 8 + 28 and K[0] == ("all",) and ("pair", 0, 7) in K
    u = np.stack([x.view(np.uint32) for x in ins])
    assert (kind[:20] == np.arange(20)).all() and (kind[20:40] == -1).all()
    assert (kind[40:400:3] == np.arange(120) % len(K)).all()
    assert (kind[41:400:3] == -1).all() and (kind[42:400:3] == -1).all()
    assert [int(u[w, 0]) for w in range(3)] == [0x7FC00001, 0x7F800002, 0xFFC00003]
    assert (u[:, 1] == 0x80000000).all() and (u[:, 3] == 1).all()
    assert [int(x) for x in u[:2, 2]] == [0x7F7FFFFF, 0xFF7FFFFF]
    e = K.index(("clash", 7, 0, 1))
    assert [int(u[w, e]) for w in (7, 0, 1)] == [0x7F800000, 0xFF800000, 0x7F800002]
    e = 40 + 3 * K.index(("pair", 2, 5))
    nan = op.is_nan(dt, np.ascontiguousarray(u[:, e]).view(np.uint8))
    assert [w for w in range(N) if nan[w]] == [2, 5]
    assert not op.is_nan(dt, ins[0])[kind == -1].any()
