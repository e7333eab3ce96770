"""Keys and inputs of the keyed consumer's tests at VPT 1, 2 and 4
(tests/test_server_tiles_gpu.py), and the tile count build_table must make of
them (tests/test_server_shapes.py checks that, and the inputs' discriminating
power, on the CPU).  A helper module (pure numpy; no torch, no GPU), not a
conftest.

Four keys per (dtype, vpt); the server's slots and store are 16-byte aligned,
so no key has a head.  A tile is 256 lanes x vpt 16-byte vectors (fold_shapes):

  key 0  1 element: element work only.
  key 1  7 elements: element work only for 1- and 2-byte types; 4- and 8-byte
         types have 1 and 3 whole vectors (a partial tile) before 3 and 1
         elements.
  key 2  one full tile of 256 * vpt vectors and 1 element.
  key 3  3 full tiles, a partial tile and a ragged tail.  The partial tile has
         300 vectors at VPT 2 (slot 1 valid on lanes 0..43) and 700 at VPT 4
         (slot 2 valid on lanes 0..187, slot 3 nowhere), the tail
         fold_shapes.ragged_tail elements.  At VPT 1 the key is
         order_probe.ragged_key (100 vectors, 5 ragged elements for 16-bit
         types); integer types, which order_probe does not know, take the
         same 3 * 256 + 100 vectors and fold_shapes.ragged_tail.

These are the smallest shapes that hold every tile kind: the largest, key 3 at
VPT 4, is 60,352 bytes (+ the tail) per worker.

Float inputs: fold_shapes.probe_inputs over fold_shapes.regions — order_probe's
probes (per-worker NaN payloads, inf clashes, -0, subnormals, +-(largest
finite)) at every third element of the first, the interior and the last full
tile, of the partial tile and of the tail (tails densely), on a finite
background; the last 16 lanes of every slot of a probed full tile stay
background.  Integer inputs are synth's ``bits`` class.  Every round has data
of its own.
"""
from __future__ import annotations

import fold_shapes as fs
import order_probe as op
from prophet_amd.dtypes import DType, FLOAT_DTYPES

_F16, _BF16, _F32, _F64 = DType.FLOAT16, DType.BFLOAT16, DType.FLOAT32, DType.FLOAT64
_U8, _I8, _I32, _I64 = DType.UINT8, DType.INT8, DType.INT32, DType.INT64

NKEYS = 4
ROUNDS = op.ROUNDS
PARTIAL_VECS = {1: 100, 2: 300, 4: 700}
ONE_TILE, RAGGED = 2, 3             # key indices

# ------------------------------------------------ the GPU tests' case lists ----
# (workers, dtype, vpt); up to 8 workers the narrow queue (the fast path's
# registers, PermSrcs in the replay and the element work), 9 to 16 the wide one
# (PermSrcs16, the second release word)
WT_NARROW = [(8, _F32, 2), (8, _F32, 4), (8, _F16, 2), (8, _F16, 4), (8, _BF16, 4), (8, _F64, 2),
             (3, _F32, 4), (2, _F16, 2)]
WT_WIDE = [(9, _F16, 2), (16, _F32, 4), (16, _BF16, 2), (12, _F64, 4)]
WT_INT = [(8, _I32, 1), (9, _U8, 1), (8, _I32, 2), (16, _I8, 4), (3, _I64, 2)]
WT = WT_NARROW + WT_WIDE + WT_INT
PLAIN = [(8, _F32, 1), (8, _F16, 2), (16, _F32, 2)]
NT = [(8, _F32, 1), (8, _F32, 2), (8, _F16, 4), (16, _BF16, 2), (8, _I32, 2)]


def case_id(case) -> str:
    return f"{case[0]}-{DType(case[1]).name}-vpt{case[2]}"


def is_float(dt) -> bool:
    return DType(dt) in FLOAT_DTYPES


# ------------------------------------------------------------------- shapes ----

def key_elems(dt, vpt: int) -> list:
    """Elements of the four keys."""
    dt = DType(dt)
    v = fs.vec_elems(dt)
    tile = fs.K_BLOCK * vpt * v
    if vpt == 1 and is_float(dt):
        ragged = op.ragged_key(dt)[0]
    else:
        ragged = 3 * tile + PARTIAL_VECS[vpt] * v + fs.ragged_tail(dt)
    return [1, 7, tile + 1, ragged]


def key_regions(dt, vpt: int, j: int) -> dict:
    """The probed element ranges of key j, by fold_shapes.regions' names."""
    return fs.regions(dt, key_elems(dt, vpt)[j], 0, vpt)


def key_tiles(dt, vpt: int, j: int) -> dict:
    """The records build_table makes of key j: {"elem", "full", "partial"}.
    One element record if any element lies outside the whole vectors (fewer
    than 4,096 of them here: one part), one record per tile of 256 * vpt
    vectors."""
    n = key_elems(dt, vpt)[j]
    nvec, tail_begin, _ = fs.geometry(dt, n)
    assert n - tail_begin <= fs.K_BLOCK * 16
    full, part = divmod(nvec, fs.K_BLOCK * vpt)
    return {"elem": int(n > tail_begin), "full": full, "partial": int(part > 0)}


def table_tiles(dt, vpt: int) -> int:
    """The tile count of the keyed table over the four keys."""
    return sum(sum(key_tiles(dt, vpt, j).values()) for j in range(NKEYS))


def slot_vecs(vpt: int) -> list:
    """Valid vectors of every slot of key 3's partial tile."""
    return [max(0, min(fs.K_BLOCK, PARTIAL_VECS[vpt] - j * fs.K_BLOCK)) for j in range(vpt)]


# ------------------------------------------------------------------- inputs ----

def inputs(dt, n_workers: int, vpt: int, rnd: int, j: int):
    """(per-worker bytes, per-element probe kind or -1) of key j in round
    `rnd`; shared, never modified."""
    n = key_elems(dt, vpt)[j]
    seed = 9000 + 1000 * vpt + 100 * rnd + 10 * j
    return op.cached(("tiles", int(dt), n_workers, vpt, rnd, j),
                     lambda: fs.probe_inputs(dt, n, n_workers, seed, key_regions(dt, vpt, j)))


def inputs_of(dt, n_workers: int, vpt: int):
    """Rig's inputs_of (tests/test_server_order_gpu.py)."""
    return lambda rnd, j: inputs(dt, n_workers, vpt, rnd, j)
