"""Shapes, layouts and inputs of the cast tests at 1, 2 and 4 units a lane
(tests/test_cast_tiles_gpu.py), and what the launch rules must make of them
(tests/test_cast_shapes.py checks that on the CPU).  A helper module (numpy
only; no torch, no GPU), not a conftest.

A cast tile is kBlock lanes x U units of 8 elements; lane l handles units
l + kBlock * j, j < U.  The plan's table builder (bpsr_cast_table.cpp build())
keeps the tuned U (Tuning::copy_vpt) only while the plan has kMinTiles tiles
or more, summed over its segments, and a segment of 8 co-aligned elements is
one partial tile at any U.  So a plan of

  main     a head of HEAD elements, full tiles, a partial tile of
           kBlock + 37 units and a tail of 5 elements,
  never    2 * kCastElemPart + 5 elements whose sides never co-align (three
           element records), and
  ballast  kMinTiles segments of 8 elements in one arena per side, 16 bytes
           of sentinel between neighbours,

is cut for U = copy_vpt while it holds some tens of thousands of elements;
without the ballast it is cut for U = 1.  The one-tensor calls have no
ballast: their U = 2 and U = 4 sizes are kMinTiles - 1 full tiles and the
partial one (`big_elems`).

The main segment is long enough (65,537 elements and more) for a 2-byte
source to hold every bit pattern, at every U.

Inputs: 2-byte sources are all 65,536 patterns in order from an odd start;
f32 / f64 sources come from `wide_table`, a shuffled table of one prime period
(ties of both wire formats and their neighbours, overflow thresholds, results
that are wire subnormals, f32 subnormals, signed zeros, infinities, NaN
payloads, f64 values that round twice, random magnitudes over 2^-30 .. 2^20),
with `edge_values` written over the positions where a tile's indexing can go
wrong (`edge_positions`).
"""
from __future__ import annotations

import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "prophet_amd", "csrc", "bpsr_internal.h")).read()
K_BLOCK = int(re.search(r"constexpr int kBlock = (\d+);", _HDR).group(1))
K_MIN_TILES = int(re.search(r"constexpr uint64_t kMinTiles = (\d+);", _HDR).group(1))
POL_NT = int(re.search(r"kPolNt = (\d+)", _HDR).group(1))
POL_WT = int(re.search(r"kPolWt = (\d+)", _HDR).group(1))
WT_MAX_MIB = int(re.search(r"kWtMaxBytes = (\d+)ull << 20", _HDR).group(1))
ELEM_PART = K_BLOCK * 16            # kCastElemPart: elements of one element record
TILE1 = K_BLOCK * 8                 # elements of a 1-unit tile
SENTINEL = 0xA5

HEAD = 3                            # elements before the main segment's vector range
TAIL = 5
PARTIAL_UNITS = K_BLOCK + 37        # the main segment's units behind its full tiles
NEVER = 2 * ELEM_PART + 5           # three element records
NSEG = K_MIN_TILES                  # ballast segments
PERIOD = 65537                      # prime: no tile repeats its neighbour's contents
ALL16 = 65536 + 1                   # a 2-byte source of this length holds every pattern

UNITS = (1, 2, 4)
WIDE_ES = {"f32": 4, "f64": 8, "x16": 2}    # x16: the other 2-byte float
WIRES = ("fp16", "bf16")

# The four processes of the GPU test: name -> (environment, BPSR_COPY_VPT or
# the default 2, BPSR_WT_MAX_MIB or -1 for the default, tile sizes it runs,
# the store policy every one of its launches must get).
ENVS = {
    "default": ({}, 2, -1, (1, 2), POL_WT),
    "u4wt": ({"BPSR_COPY_VPT": "4", "BPSR_WT_MAX_MIB": "1024"}, 4, 1024, (4,), POL_WT),
    "nt": ({"BPSR_WT_MAX_MIB": "0"}, 2, 0, (1, 2), POL_NT),
    "u4nt": ({"BPSR_COPY_VPT": "4", "BPSR_WT_MAX_MIB": "0"}, 4, 0, (4,), POL_NT),
}


def cases(env: str) -> list:
    """(entry, U, wide element size, scheme) of every launch shape the GPU
    test's process `env` runs; each plain one is compressed and decompressed.
    The error-feedback and stochastic-rounding compresses take f32 only and
    run through the ballast plan."""
    out = []
    for u in ENVS[env][3]:
        for es in (4, 8, 2):
            out += [("single", u, es, "plain"), ("plan", u, es, "plain")]
        if u > 1:
            out += [("plan", u, 4, "ef"), ("plan", u, 4, "sr")]
    return out


def offsets(k: int, es: int):
    """tests/test_cast_stats_gpu.py's _offsets: byte offsets past a 16-byte
    boundary of the wide and the 2-byte operand that co-align after k
    elements."""
    from test_cast_stats_gpu import _offsets      # imported late: that module needs torch
    return _offsets(k, es)


# ------------------------------------------------------------------ shapes ----

def full_tiles(u: int) -> int:
    """Full tiles of u units a lane in the main segment: 3 or more, and enough
    for ALL16 elements with the partial tile."""
    need = ALL16 - PARTIAL_UNITS * 8
    return max(3, -(-need // (u * TILE1)))


def main_elems(u: int) -> int:
    return HEAD + full_tiles(u) * u * TILE1 + PARTIAL_UNITS * 8 + TAIL


def big_elems(u: int) -> int:
    """The one-tensor call that keeps u units a lane: kMinTiles tiles, the
    last one partial."""
    return HEAD + (K_MIN_TILES - 1) * u * TILE1 + PARTIAL_UNITS * 8 + TAIL


def single_elems(u: int) -> int:
    return main_elems(1) if u == 1 else big_elems(u)


def main_segment(u: int, k: int = HEAD, n: int | None = None) -> dict:
    """The layout of a main segment of n elements (main_elems(u) unless given)
    as a table cut for u must see it: head, full tiles, the partial tile's
    units, tail, and the first element of each."""
    n = main_elems(u) if n is None else n
    units = (n - k) // 8
    tile = K_BLOCK * u
    full, partial = units // tile, units % tile
    return {"n": n, "head": k, "full": full, "partial": partial,
            "tail": n - k - 8 * units, "partial_at": k + full * tile * 8,
            "tail_at": k + 8 * units, "u": u}


def segments(u: int, kind: str = "plan") -> list:
    """(name, elements, head or None) of every segment of a GPU case: the plan
    cut for u, or ("single") the one-tensor call."""
    if kind == "single":
        return [("main", single_elems(u), HEAD)]
    segs = [("main", main_elems(u), HEAD), ("never", NEVER, None)]
    if u > 1:
        segs += [("ballast", 8, 0)] * NSEG
    return segs


def layout(segs: list, es: int):
    """Byte offsets of every segment in one arena per side (wide, 2-byte), from
    a 256-byte aligned base, and the arenas' sizes.  Ballast segments are
    16-byte aligned with 16 sentinel bytes between them; every other segment
    starts at its co-alignment offsets past a 256-byte boundary, 256 sentinel
    bytes and more in front of it."""
    pos = [256, 256]
    offs = ([], [])
    for name, n, k in segs:
        if name == "ballast":
            add, gap, al = (0, 0), 16, 16
        else:
            add, gap, al = (offsets(k, es) if k is not None else (0, 2)), 256, 256
        for side, width in ((0, es), (1, 2)):
            p = -(-pos[side] // al) * al + add[side]
            offs[side].append(p)
            pos[side] = p + n * width + gap
    return offs[0], offs[1], pos[0] + 256, pos[1] + 256


def edge_positions(m: dict) -> list:
    """Element indices of a main segment where an indexing error shows: first
    and last of the head, lane 0 and lane kBlock - 1 of the first and last j of
    every full tile (first and last element of the unit), the partial tile's
    first unit, its last lane of j = 0, its first and last unit of j = 1 (the
    last live one), and the tail."""
    u, k = m["u"], m["head"]
    pos = [0, k - 1] if k else []
    for t in range(m["full"]):
        t0 = k + t * u * TILE1
        for j in sorted({0, u - 1}):
            for lane in (0, K_BLOCK - 1):
                e = t0 + (j * K_BLOCK + lane) * 8
                pos += [e, e + 7]
    p0, live = m["partial_at"], m["partial"]
    for unit in sorted({0, min(live, K_BLOCK) - 1, min(live - 1, K_BLOCK), live - 1}):
        pos += [p0 + unit * 8, p0 + unit * 8 + 7]
    pos += list(range(m["tail_at"], m["n"]))
    return [p for p in dict.fromkeys(pos) if 0 <= p < m["n"]]


# ------------------------------------------------------------------ inputs ----

def patterns16(n: int, start: int = 0x3c01) -> np.ndarray:
    """n 2-byte patterns in order from an odd start (uint16)."""
    assert start % 2 == 1
    return ((np.arange(n, dtype=np.int64) + start) & 0xffff).astype(np.uint16)


_NAN32 = [0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0x7f801fff]
_NAN64 = [0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000001,
          0x7fffffffffffffff, 0x7ff0000020000000]


def _specials() -> np.ndarray:
    """The finite and infinite kinds, as f64 values that f32 holds exactly."""
    f32 = np.float32
    inf = f32(np.inf)
    # fp16 ties and their f32 neighbours: a sample of every finite magnitude,
    # the subnormal results, the first normals and the last (65504 | 65536)
    hb = np.unique(np.concatenate([np.arange(0, 0x7c00, 61), np.arange(0, 40),
                                   np.arange(0x3f0, 0x410), np.arange(0x7bf0, 0x7c00)]))
    hb = hb.astype(np.uint16)
    lo = hb.view(np.float16).astype(np.float64)
    hi = (hb + np.uint16(1)).view(np.float16).astype(np.float64)
    hi[-1] = 65536.0
    mid = ((lo + hi) / 2).astype(f32)
    f16 = np.concatenate([mid, np.nextafter(mid, inf), np.nextafter(mid, -inf)])
    # bf16 ties (f32 bits ....8000) and their neighbours, f32 subnormals included
    top = np.unique(np.concatenate([np.arange(0, 0x7f80, 53), np.arange(0, 0x100),
                                    np.arange(0x7f70, 0x7f80)])).astype(np.uint32)
    tie = (top << np.uint32(16)) | np.uint32(0x8000)
    bf = np.concatenate([tie, tie + np.uint32(1), tie - np.uint32(1)]).view(f32)
    # tests/test_compress_gpu.py _structured_f32, tests/test_cast_plan_gpu.py _values
    named = np.array([65504.0, 65519.996, 65520.0, 65536.0, 1e38, 0.0, np.inf, 7e4, 1e-7, 3e-8,
                      2.0 ** -25, 2.0 ** -24 * 1.5, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 6.1e-5,
                      6.0e-5, 2049.0, 2051.0, 4098.0, 3.0, 1 / 3, 65519.0, 3.3e38, 3.4e38], f32)
    sub = np.array([1, 2, 0x7fffff, 0x400000, 0x800000], np.uint32).view(f32)
    pos = np.concatenate([f16, bf, named, sub]).astype(np.float64)
    return np.concatenate([pos, -pos])


def _twice() -> np.ndarray:
    """f64 values that round twice on the way through f32: to fp16 1.0 and not
    1 + 2^-10, to bf16 1.0 and not 1 + 2^-7; and what f32 turns into 0 or inf."""
    t = np.array([1 + 2.0 ** -11 + 2.0 ** -30, 1 + 2.0 ** -8 + 2.0 ** -30,
                  3 * (1 + 2.0 ** -11 + 2.0 ** -35), 2.0 ** -14 * (1 + 2.0 ** -11 + 2.0 ** -40),
                  65519.99999, 1e-300, 1e300, 2.0 ** -150, 2.0 ** -149 * 1.5])
    return np.concatenate([t, -t])


@functools.lru_cache(maxsize=None)
def wide_table(es: int, seed: int = 77) -> np.ndarray:
    """PERIOD source values of the wide type (4: float32, 8: float64), as that
    numpy dtype, shuffled so that any stretch holds every kind.  Shared: read
    only."""
    dt, ut, nans = (np.float32, np.uint32, _NAN32) if es == 4 else (np.float64, np.uint64, _NAN64)
    rng = np.random.default_rng(seed)
    vals = _specials() if es == 4 else np.concatenate([_specials(), _twice()])
    nrand = PERIOD - len(vals) - len(nans)
    assert nrand > PERIOD // 2
    rnd = np.exp2(rng.uniform(-30.0, 20.0, nrand)) * rng.choice([-1.0, 1.0], nrand)
    with np.errstate(over="ignore", under="ignore"):
        out = np.concatenate([vals, rnd, np.zeros(len(nans))]).astype(dt)
    out.view(ut)[-len(nans):] = np.array(nans, ut)
    out = out[rng.permutation(PERIOD)]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edge_values(es: int) -> np.ndarray:
    """The values written over `edge_positions`, in turn: a NaN, infinities,
    signed zeros, the overflow threshold and its neighbours, ties, a result
    that is a wire subnormal, an f32 subnormal, and for f64 a value that rounds
    twice."""
    dt, ut, nans = (np.float32, np.uint32, _NAN32) if es == 4 else (np.float64, np.uint64, _NAN64)
    v = [0.0, np.inf, -np.inf, 0.0, -0.0, 65520.0, 65519.996, -65504.0, 1 + 2.0 ** -11,
         -(1 + 3 * 2.0 ** -11), 1 + 2.0 ** -8, 3e-8, -2.0 ** -25, 2.0 ** -140, 0.0, -7e4, 3.39e38]
    if es == 8:
        v += [1 + 2.0 ** -11 + 2.0 ** -30, -(1 + 2.0 ** -8 + 2.0 ** -30), 1e-300]
    out = np.array(v, dt)
    out.view(ut)[0] = nans[2]                     # a signalling payload
    out.view(ut)[14] = nans[1]
    out.setflags(write=False)
    return out


def edge_index(m: dict, es: int):
    """(positions, which edge value goes there): the values in turn, shifted
    by one each time round so that a position's kind varies from tile to tile."""
    pos = np.array(edge_positions(m), np.int64)
    i = np.arange(len(pos))
    turn = len(edge_values(es))
    return pos, (i + i // turn) % turn


def wide_source(es: int, m: dict | None, n: int, shift: int = 0) -> np.ndarray:
    """n source values of the wide type: the table from entry `shift` on,
    repeated, the edge values over a main segment's edge positions."""
    x = np.take(wide_table(es), (np.arange(n) + shift) % PERIOD)
    if m is not None:
        pos, which = edge_index(m, es)
        x[pos] = edge_values(es)[which]
    return x


def plan_values(src_es: int, segs: list, u: int) -> np.ndarray:
    """The source values of every segment of `segs`, one after the other:
    2-byte patterns (uint16) for src_es == 2, else the wide type's table, each
    segment from a place of its own, the main segment with its edge values."""
    parts = []
    for i, (name, n, k) in enumerate(segs):
        if src_es == 2:
            parts.append(patterns16(n, (0x3c01 + 74 * i) & 0xffff))
        else:
            m = main_segment(u, k, n) if name == "main" else None
            parts.append(wide_source(src_es, m, n, 997 * i))
    return np.concatenate(parts)
