"""Shapes and inputs of the reference-mode fold tests at the real tile sizes
(tests/test_fold_tiles_gpu.py, tests/test_fold_policy_gpu.py, and with
operands that are one buffer tests/test_fold_alias_gpu.py), and what the
launch rules must make of them (tests/test_fold_shapes.py checks that on the
CPU).  A helper module (pure numpy; no torch, no GPU), not a conftest.

A tile is 256 lanes x VPT 16-byte vectors; lane l of a tile handles vectors
l + 256 j, j < VPT ("slot j").  fold_vpt (bpsr_internal.h) keeps the tuned VPT
only from kMinTiles = 2048 tiles on, so the shapes are the smallest that keep
VPT 2 and VPT 4:

  V2  2047 * 512 + 300 vectors: 2048 tiles at VPT 2; the last one is partial
      with 300 vectors — slot 0 valid on every lane, slot 1 on lanes 0..43.
  V4  2047 * 1024 + 700 vectors: 2048 tiles at VPT 4; the partial one has
      slots 0 and 1 full, slot 2 valid on lanes 0..187, slot 3 invalid.
  SMALL  3 full tiles at VPT 1, 100 vectors and the tail (test_accum_gpu).

Element counts add a ragged tail behind the last whole vector: 3 elements
(1 for 8-byte types, 5 for 1-byte types); for fp16 those are the F16C scalar
tail.  With `head` elements before the first whole vector (operands co-aligned
at a byte offset) fp16 gets the rest of a vector more, so that the element
count stays 3 mod 8 and the vector count stays what the shape says.

Inputs: a finite background (a few tiles of order_probe's background, repeated
with a period that is no multiple of a tile) and order_probe's probes — NaNs
with a payload per source, inf clashes, -0, subnormals, +-(largest finite) at
every third element — over the head, the first full tile, one interior full
tile, the last full tile, the partial tile and the tail.  The last 16 lanes of
every slot of a probed full tile stay background, so each slot holds vectors
that go to the NaN replay and vectors that do not; every other tile is finite.
Integer dtypes hold synth's ``bits`` class throughout.
"""
from __future__ import annotations

import numpy as np

import order_probe as op
from prophet_amd import synth
from prophet_amd.dtypes import DType, FLOAT_DTYPES, elem_size

K_BLOCK = 256                       # bpsr_internal.h kBlock
K_MIN_TILES = 2048                  # bpsr_internal.h kMinTiles
POL_PLAIN, POL_NT, POL_WT = 0, 1, 2   # bpsr_internal.h kPolPlain / kPolNt / kPolWt

# name -> (16-byte vectors per operand, the VPT the launch rules must choose)
SHAPES = {
    "V2": (2047 * 512 + 300, 2),
    "V4": (2047 * 1024 + 700, 4),
    "SMALL": (3 * 256 + 100, 1),
}

_F32, _F64, _F16, _BF16 = DType.FLOAT32, DType.FLOAT64, DType.FLOAT16, DType.BFLOAT16
_U8, _I8, _I32, _I64 = DType.UINT8, DType.INT8, DType.INT32, DType.INT64

# ------------------------------------------------ the GPU tests' case lists ----
# byteps_reduce_sum_n, separate dst: (dtype, sources, shape)
_FLOAT_CASES = [(2, "V4"), (3, "V2"), (8, "V2"), (8, "V4"), (9, "V2"), (16, "V2")]
_INT_CASES = [(2, "V4"), (8, "V2"), (9, "V4")]
SUM_N = ([(dt, n, s) for dt in (_F32, _F64, _F16, _BF16) for n, s in _FLOAT_CASES]
         + [(dt, n, s) for dt in (_F32, _F16) for n, s in ((9, "V4"), (16, "V4"))]
         + [(dt, n, s) for dt in (_U8, _I32, _I64) for n, s in _INT_CASES])
IN_PLACE = [(dt, 8, "V2") for dt in (_F32, _F64, _F16, _BF16)] + [(_F32, 3, "V4")]
# (dtype, sources, shape, byte offset of every operand inside its 16-byte line)
OFFSET = [(dt, 8, "V2", 8) for dt in (_F32, _F64, _F16, _BF16)] + [(_I32, 2, "V4", 4)]
POLICY_SMALL_N = [2, 8, 9, 16]
POLICY_BIG = [(_F32, 8, "V2"), (_F16, 8, "V2")]
POLICY_NT_EXTRA = [(_F32, 8, "V4")]
BATCH_DTYPES = [_F32, _F16, _F64, _I8]
BLOCKQ_DTYPES = [_F32, _F16, _BF16, _F64, _I32]
# the policy tests' block queue: the tile size is the fold rule's own
POLICY_BLOCKQ_DTYPES = [_F32, _F16]
POLICY_BLOCKQ_VPT = 1


# Aliased operands (tests/test_fold_alias_gpu.py): (dtype, sources, shape, the
# source index that dst is or None, groups of source indices in one buffer).
_DUP_CASES = [(3, "V4"), (8, "V2"), (9, "V2"), (16, "V2")]


def _dup_groups(n: int, first: int) -> tuple:
    """A neighbouring pair from source `first` on; above 8 sources also a
    pair whose second member lies in the second load group."""
    return ((first, first + 1),) + (((first + 2, n - 1),) if n > 8 else ())


# sum_n(dst, [a, a, b, ...]) and sum_n(a, [a, b, b, ...])
ALIAS_DUP = [(dt, n, s, alias, _dup_groups(n, 0 if alias is None else 1))
             for dt in (_F32, _F16, _BF16) for n, s in _DUP_CASES for alias in (None, 0)]
# dst is srcs[k], k > 0 (fold_any_alias; the shard ABI alone gets there):
# reduce_scatter in place at world 3 (k = rank), reduce_root in place at
# world 8 with root 5, and landed pushes folded into one of them, where k lies
# in the second load group of the tiles and of fold_elements
ALIAS_SCATTER = [(dt, 3, "V4", k, ()) for dt in (_F32, _F16) for k in (1, 2)]
ALIAS_ROOT = [(dt, 8, "V2", 5, ()) for dt in (_F16, _BF16, _F64)]
ALIAS_LANDED = ([(dt, 9, "V2", 8, ()) for dt in (_F32, _F16)]
                + [(dt, 12, "SMALL", 9, ()) for dt in (_F32, _F16, _BF16)])
ALIAS = ALIAS_DUP + ALIAS_SCATTER + ALIAS_ROOT + ALIAS_LANDED
# byteps_reduce_sum3 and byteps_reduce_sum(dst, dst): two sources
SUM3_DTYPES = [_F32, _F64, _F16, _BF16, _I32, _U8, _I64]
SUM3_CASES = ([(dt, 2, "V4") for dt in SUM3_DTYPES] + [(dt, 2, "SMALL") for dt in (_F16, _F32)]
              + [(dt, 2, "SMALL", 8) for dt in (_F16, _F32)])
DOUBLING = [(dt, 2, "V4") for dt in (_F32, _F16, _I32)]


def case_id(case) -> str:
    dt, n, shape = case[:3]
    return f"{DType(dt).name}-n{n}-{shape}" + (f"-off{case[3]}" if len(case) > 3 else "")


def alias_id(case) -> str:
    dt, n, shape, alias, same = case
    return (case_id((dt, n, shape)) + ("" if alias is None else f"-dst{alias}")
            + "".join("-same" + "_".join(map(str, g)) for g in same))


def ns_kernel(n: int) -> int:
    """fold_kernel's compile-time source count (launch_fold_vpt): 2, 8, 16 or
    0, the generic kernel."""
    return n if n in (2, 8, 16) else 0


# ----------------------------------------------------------------- geometry ----

def vec_elems(dt) -> int:
    return 16 // elem_size(dt)


def ragged_tail(dt) -> int:
    return {1: 5, 2: 3, 4: 3, 8: 1}[elem_size(dt)]


def head_elems(dt, off: int) -> int:
    """Elements before the first whole vector of operands `off` bytes past a
    16-byte boundary."""
    assert off % elem_size(dt) == 0 and 0 <= off < 16
    return ((16 - off) % 16) // elem_size(dt)


def n_elems(dt, vecs: int, head: int = 0) -> int:
    n = head + vecs * vec_elems(dt) + ragged_tail(dt)
    if head and DType(dt) == _F16:
        n += vec_elems(dt) - head
    return n


def geometry(dt, n: int, head: int = 0):
    """(vectors, first element behind them, first fp16 scalar-tail element):
    make_geom (bpsr_table.cpp) for co-aligned operands."""
    v = vec_elems(dt)
    body = n // 8 * 8 if DType(dt) == _F16 else n
    nvec = (body - head) // v if body > head else 0
    return nvec, head + nvec * v, body


def regions(dt, n: int, head: int, vpt: int) -> dict:
    """The probed element ranges of a bucket of n elements folded in tiles of
    256 * vpt vectors, by name; a range the bucket does not have is left out."""
    v = vec_elems(dt)
    nvec, tail_begin, body = geometry(dt, n, head)
    t = K_BLOCK * vpt * v
    full = nvec // (K_BLOCK * vpt)
    reg = {}
    if head:
        reg["head"] = (0, head)
    if full >= 1:
        reg["first_tile"] = (head, head + t)
    if full >= 3:
        mid = full // 2
        reg["interior_tile"] = (head + mid * t, head + (mid + 1) * t)
    if full >= 2:
        reg["last_full_tile"] = (head + (full - 1) * t, head + full * t)
    if tail_begin > head + full * t:
        reg["partial_tile"] = (head + full * t, tail_begin)
    if body > tail_begin:           # behind the last vector, the body's NaN rule
        reg["tail"] = (tail_begin, body)
    if body < n:                    # fp16's scalar tail, a range of its own: it begins with `all`
        reg["scalar_tail"] = (body, n)
    return reg


def slot(dt, reg: tuple, j: int) -> tuple:
    """Elements of slot j (vectors 256 j .. 256 j + 255) of the tile that
    begins at reg[0], clipped to reg."""
    lo = reg[0] + j * K_BLOCK * vec_elems(dt)
    return min(lo, reg[1]), min(lo + K_BLOCK * vec_elems(dt), reg[1])


# ------------------------------------------------------------------- inputs ----
BG_VECS = 3 * 256 + 37              # the background's period, in vectors
FINITE_LANES = 16                   # of every slot of a probed full tile
FULL_TILES = ("first_tile", "interior_tile", "last_full_tile")


def finite_lanes(dt, name: str, lo: int, hi: int) -> list:
    """The element ranges of a probed full tile that stay background: the last
    FINITE_LANES lanes of every slot (16-bit types hold a probe in every
    vector otherwise), so that each slot has vectors that are replayed and
    vectors whose fast result is stored."""
    if name not in FULL_TILES:
        return []
    c, keep = K_BLOCK * vec_elems(dt), FINITE_LANES * vec_elems(dt)
    return [(a + c - keep, a + c) for a in range(lo, hi, c)]


def _background(dt, n: int, n_src: int, seed: int, cls=None):
    """n elements per source as bit patterns: BG_VECS vectors repeated."""
    U = np.dtype(f"u{elem_size(dt)}")
    period = min(n, BG_VECS * vec_elems(dt))
    if n == 0:
        return np.zeros((n_src, 0), U)
    if cls is None:
        rows = [x.view(U) for x in op.inputs(dt, period, n_src, seed, [])[0]]
    else:
        rows = [np.ascontiguousarray(synth.bucket(dt, period, k, cls, seed)).view(U)
                for k in range(n_src)]
    return np.stack([np.resize(r, n) for r in rows])


def probe_inputs(dt, n: int, n_src: int, seed: int, reg: dict, cls: str = "bits"):
    """(per-source byte arrays, per-element probe kind or -1) of a bucket of n
    elements.  Float dtypes with two sources or more: the finite background
    with order_probe's probes over every range of `reg`.  Integer dtypes and
    single sources: synth's class `cls`, no probes."""
    dt = DType(dt)
    kind = np.full(n, -1, np.int32)
    if dt not in FLOAT_DTYPES or n_src < 2:
        data = _background(dt, n, n_src, seed, cls)
    else:
        data = _background(dt, n, n_src, seed)
        for i, (name, (lo, hi)) in enumerate(reg.items()):
            if hi <= lo:
                continue
            ins, k = op.inputs(dt, hi - lo, n_src, seed + 17 * (i + 1), [(0, hi - lo)])
            keep = [(a, data[:, a:b].copy()) for a, b in finite_lanes(dt, name, lo, hi)]
            for w in range(n_src):
                data[w, lo:hi] = ins[w].view(data.dtype)
            kind[lo:hi] = k
            for a, saved in keep:
                data[:, a:a + saved.shape[1]] = saved
                kind[a:a + saved.shape[1]] = -1
    return [np.ascontiguousarray(data[w]).view(np.uint8) for w in range(n_src)], kind


def oracle_fold(dt, ins, L: int) -> np.ndarray:
    """The oracle's left fold of `ins` in their order: L bytes (trailing bytes
    past the last whole element come from ins[0], as in the server's fold)."""
    from oracle.oracle import PortReducer
    want = np.zeros(L, np.uint8)
    if L:
        assert PortReducer(nthreads=8).sum_n(want, list(ins), L, dt) == 0
    return want


# A few cases are used by more than one test (separate dst and in place, both
# cache policies): the latest entries are kept, up to a byte budget.
_KEPT: dict = {}
_KEEP_BYTES = 1 << 30


def fold_case(dt, n_src: int, shape: str, off: int = 0):
    """(sources, kinds, expected bytes, regions) of one sum_n case; shared,
    never modified."""
    key = (int(dt), n_src, shape, off)
    if key not in _KEPT:
        vecs, vpt = SHAPES[shape]
        head = head_elems(dt, off)
        n = n_elems(dt, vecs, head)
        reg = regions(dt, n, head, vpt)
        ins, kind = probe_inputs(dt, n, n_src, 4000 + 10 * n_src + off, reg)
        want = oracle_fold(dt, ins, n * elem_size(dt))
        _KEPT[key] = (ins, kind, want, reg)
        size = lambda v: sum(a.nbytes for a in v[0]) + v[1].nbytes + v[2].nbytes  # noqa: E731
        while len(_KEPT) > 1 and sum(size(v) for v in _KEPT.values()) > _KEEP_BYTES:
            _KEPT.pop(next(iter(_KEPT)))
    return _KEPT[key]


def share(ins: list, same) -> list:
    """`ins` with every member of a group of `same` replaced by the group's
    first input, the same array object: duplicates share their input."""
    out = list(ins)
    for group in same:
        for k in group[1:]:
            out[k] = out[group[0]]
    return out


_ALIAS_WANT: dict = {}


def alias_case(case):
    """(sources, kinds, expected bytes, regions) of a case of ALIAS: fold_case's
    inputs with the duplicates sharing theirs, and the oracle's fold of that
    list (which holds the same array twice for a duplicate).  Which source dst
    is does not enter: the fold is element-wise."""
    dt, n, shape, _, same = case
    ins, kind, want, reg = fold_case(dt, n, shape)
    if not same:
        return ins, kind, want, reg
    ins = share(ins, same)
    key = (int(dt), n, shape, same)
    if key not in _ALIAS_WANT:
        _ALIAS_WANT[key] = oracle_fold(dt, ins, len(want))
    return ins, kind, _ALIAS_WANT[key], reg


def scatter_vectors(dt, world: int, shape: str, seed: int):
    """Every rank's whole vector for a reduce_scatter whose owned slices have
    `shape` each: (E, per-rank byte arrays, kinds, per-owner byte offset inside
    the 16-byte line).  E = world * n_elems(shape), so owner q's slice begins
    at (q * n_elems * element size) % 16: probes are placed per slice, for the
    head that offset gives (regions)."""
    es = elem_size(dt)
    vecs, vpt = SHAPES[shape]
    per = n_elems(dt, vecs)
    E = world * per
    parts, kinds, offs = [], [], []
    for q in range(world):
        off = (q * per * es) % 16
        reg = regions(dt, per, head_elems(dt, off), vpt)
        ins, kind = probe_inputs(dt, per, world, seed + q, reg)
        parts.append(ins)
        kinds.append(kind)
        offs.append(off)
    full = [np.concatenate([parts[q][r] for q in range(world)]) for r in range(world)]
    return E, full, np.concatenate(kinds), offs


# ------------------------------------------------------------------- tables ----
# The ragged table of test_parity_gpu.test_batched_ragged_mixed_table:
# (elements, sources, byte offsets of dst + sources or None, class of the
# buckets without probes), offsets in units of the element size where marked.
def ragged_spec(dt) -> list:
    es = elem_size(dt)
    return [
        (100_000, 8, None, "special"), (4099, 9, None, "normal"), (1, 1, None, "normal"),
        (70_001, 32, None, "bits"), (0, 8, None, "normal"), (3 * 1024 + 5, 2, [4, 4, 4], "normal"),
        (50_000, 3, [0, es, 2 * es, 1], "normal"), (257, 12, None, "special"),
        (300_000, 5, [2, 6, 10, 14, 2, 6], "normal"), (9, 8, None, "bits"),
    ]


TRAILING_BUCKET = 3                 # this bucket's length has 3 bytes more
BALLAST_VECS = {2: 2047 * 512, 4: 2047 * 1024}


def table_spec(dt, vpt: int) -> list:
    """ragged_spec plus the two-source ballast bucket that brings the table to
    VPT `vpt` (1: no ballast)."""
    spec = ragged_spec(dt)
    if vpt > 1:
        spec.append((BALLAST_VECS[vpt] * vec_elems(dt), 2, None, "normal"))
    return spec


def bucket_offsets(offs, n_src: int) -> list:
    """Byte offsets of dst and the n_src sources."""
    offs = list(offs) if offs else [0] * (n_src + 1)
    return (offs + [offs[-1]] * (n_src + 1))[:n_src + 1]


def bucket_head(dt, offs, n_src: int):
    """Head elements of a bucket at `offs`, or None where the operands are not
    co-aligned and element-aligned (element work only)."""
    o = bucket_offsets(offs, n_src)
    es = elem_size(dt)
    if any(x % es for x in o) or len({x % 16 for x in o}) > 1:
        return None
    return head_elems(dt, o[0] % 16)


def bucket_regions(dt, n: int, offs, n_src: int, vpt: int) -> dict:
    head = bucket_head(dt, offs, n_src)
    if head is None or head > n:
        return {"elements": (0, n)}
    return regions(dt, n, head, vpt)


# Duplicated sources of the tables (bucket index, in ragged_spec and in the
# block queue's MIXED alike -> groups): the 8-source bucket of the register
# path and the 9-source one of the pointer-array path, there across its two
# load groups.
TABLE_DUPS = {0: ((0, 1),), 1: ((2, 8),)}


def table_inputs(dt, spec: list, vpt: int, seed: int, dups=None):
    """Per bucket of `spec`: (sources, kinds, expected bytes); bucket
    TRAILING_BUCKET gets 3 trailing bytes per source.  `dups`: bucket index ->
    groups of sources that share one input (share)."""
    out = []
    for i, (ne, n_src, offs, cls) in enumerate(spec):
        reg = bucket_regions(dt, ne, offs, n_src, vpt)
        ins, kind = probe_inputs(dt, ne, n_src, seed + i, reg, cls)
        if i == TRAILING_BUCKET:
            ins = [np.concatenate([x, np.array([k, 7, 9], np.uint8)]) for k, x in enumerate(ins)]
        ins = share(ins, (dups or {}).get(i, ()))
        out.append((ins, kind, oracle_fold(dt, ins, len(ins[0]))))
    return out


# The block queue's buckets: test_blockq_gpu.MIXED with the byte offsets the
# ragged table gives the same buckets.
def blockq_blocks() -> list:
    from test_blockq_gpu import MIXED       # imported late: that module needs torch
    return MIXED


def blockq_offsets(dt, ne: int, n_src: int):
    for e, n, offs, _ in ragged_spec(dt):
        if (e, n) == (ne, n_src):
            return offs
    return None
