// 1-bit sign compression with error feedback (byteps_reduce_onebit_*,
// DESIGN.md §11.10; the definition is prophet_amd/onebit.py).  What the host
// side (bpsr_onebit.cpp: operand checks, tables, the C entry points) and the
// kernels (bpsr_k_onebit.hip) share: the payload's layout, the two tables'
// records and the launches.
//
// A payload is a 16-byte header {f32 scale, u32 n_lo, u32 n_hi, u32 0} and
// ceil(n / 64) u64 words, bit k of word w the sign of element 64 w + k.
//
// A compress is three launches over one table of tiles: ACCUMULATE writes
// c = g + r over r and leaves one f64 partial of sum |c| per wave, FINISH adds
// each segment's partials up in a fixed order and writes its header, PACK
// reads the scale from the header, writes r' = c -/+ scale and the bit words.
// A fold is one launch over a table of per-wave records.  A refold (the server
// round) is a compress whose first pass folds N payloads in
// registers in place of reading a gradient.
#pragma once

#include "bpsr_internal.h"

namespace bpsr {

constexpr uint64_t kOneBitHeader = 16;
// A compress tile: kBlock lanes x 4 b128 vectors of g and of r, 4,096 elements
// (64 words) a workgroup, 1,024 (16 words) a wave.  A fold record: 64 words a
// WAVE, so a workgroup runs kBlock / 64 records.  Both start on a multiple of
// 64 elements of their segment: no word is shared between two of them.
constexpr uint32_t kOneBitTile = kBlock * 16;
constexpr uint32_t kOneBitWaves = kBlock / 64;
constexpr int kOneBitMaxSrcs = 16;
// a record's first word is a 32-bit index into its payload
constexpr uint64_t kOneBitMaxElems = 1ull << 37;

inline uint64_t onebit_words(uint64_t nelem) { return (nelem + 63) / 64; }
inline uint64_t onebit_payload_bytes(uint64_t nelem) {
  return kOneBitHeader + 8 * onebit_words(nelem);
}

// One tile of a compress (a workgroup) or of a fold (a wave): both pointers
// already advanced to the tile's first element.
enum : uint32_t { kOneBitVec = 1, kOneBitAligned = 2 };
struct OneBitRec {
  unsigned char* a;  // compress: the gradient; fold: the output
  unsigned char* b;  // compress: the residual; fold: null
  uint32_t seg;      // the segment (OneBitSeg, and the fold's row of sources)
  uint32_t word0;    // the tile's first word in its segment's payloads
  uint32_t count;    // elements, 1..kOneBitTile
  uint32_t flags;    // kOneBitVec: a and b 16-byte aligned; kOneBitAligned: 4-byte aligned
};
static_assert(sizeof(OneBitRec) == 32, "OneBitRec layout");

// One segment of a compress plan: its payload and, for FINISH, its tiles —
// records [rec_begin, rec_begin + nrecs), each with kOneBitWaves partials.
struct OneBitSeg {
  unsigned char* payload;
  uint64_t nelem;
  uint32_t rec_begin, nrecs;
  uint64_t pad;
};
static_assert(sizeof(OneBitSeg) == 32, "OneBitSeg layout");

struct OneBitCompress {
  const OneBitRec* recs;
  const OneBitSeg* segs;
  double* part;  // [nrecs * kOneBitWaves]
  uint32_t nrecs, nsegs;
};

struct OneBitFold {
  const OneBitRec* recs;
  const unsigned char* const* srcs;  // [nsegs * nsrc] payloads, a segment's row in argument order
  uint32_t nrecs;
  int nsrc;
  int divisor;
};

// The server round (bpsr_k_onebit_refold.hip): a compress whose input is the
// fold of `nsrc` payloads.  It runs over the compress table — a record's `b`
// the residual tile, `a` unused, `seg` also the row of sources — and leaves
// the compress's partials.
struct OneBitRefold {
  OneBitCompress c;
  const unsigned char* const* srcs;  // [nsegs * nsrc], as OneBitFold::srcs
  int nsrc;
};

// ACCUMULATE, FINISH and PACK on `s`; `resid_bytes`: what ACCUMULATE writes
// (store policy).
hipError_t launch_onebit_compress(const OneBitCompress& p, uint64_t resid_bytes, const Tuning& tu,
                                  hipStream_t s);
// FINISH and PACK alone, after a first pass on `s`.
hipError_t launch_onebit_finish_pack(const OneBitCompress& p, uint64_t resid_bytes,
                                     const Tuning& tu, hipStream_t s);
// REFOLD-ACCUMULATE, FINISH and PACK on `s`.
hipError_t launch_onebit_refold(const OneBitRefold& p, uint64_t resid_bytes, const Tuning& tu,
                                hipStream_t s);
// The fold; `out_bytes`: what it writes (store policy).
hipError_t launch_onebit_fold(const OneBitFold& p, uint64_t out_bytes, const Tuning& tu,
                              hipStream_t s);

}  // namespace bpsr
