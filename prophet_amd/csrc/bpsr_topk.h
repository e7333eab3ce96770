// Top-k sparsification with error feedback (byteps_reduce_topk_*, DESIGN.md
// §11.12; the definition is prophet_amd/topk.py).  What the host side
// (bpsr_topk.cpp: operand checks, tables, the C entry points) and the kernels
// (bpsr_k_topk.hip) share: the payload's layout, the tables' records, the
// plan-owned scratch and the launches.
//
// A payload is a 16-byte header {u32 k, u32 n_lo, u32 n_hi, u32 0}, k u32
// indices, strictly ascending, and k f32 values.
//
// A compress is a radix select over key = bits(c) & 0x7fffffff, 31 bits cut
// into digits of 11, 10 and 10 bits, and a stable compaction; ten launches over
// one table of tiles, ordered by the stream alone:
//   ZERO, ACCUMULATE-HISTOGRAM, PICK 0, REFINE 1, PICK 1, REFINE 2, PICK 2,
//   COUNT, SCAN, COMPACT
// A fold is one launch over a table of output tiles.  A refold — the server
// round — is the compress's ten with the fold fused into the second.
#pragma once

#include "bpsr_internal.h"

namespace bpsr {

constexpr uint64_t kTopKHeader = 16;
// A tile: kBlock lanes x 4 b128 vectors, 4,096 elements a workgroup; vector
// j * kBlock + lane is lane's j-th, so a wave's j-th load is 1 KiB contiguous.
constexpr uint32_t kTopKTile = kBlock * 16;
constexpr uint32_t kTopKWaves = kBlock / 64;
constexpr int kTopKMaxSrcs = 16;
constexpr uint64_t kTopKMaxElems = 1ull << 31;
// the digits of the 31-bit key, most significant first
constexpr uint32_t kTopKBits0 = 11, kTopKBits1 = 10, kTopKBits2 = 10;
constexpr uint32_t kTopKBins = (1u << kTopKBits0) + (1u << kTopKBits1) + (1u << kTopKBits2);

inline uint64_t topk_payload_bytes(uint64_t k) { return kTopKHeader + 8 * k; }

// One tile of a compress or of a fold: both pointers already advanced to the
// tile's first element.
enum : uint32_t { kTopKVec = 1, kTopKAligned = 2 };
struct TopKRec {
  unsigned char* a;  // compress: the gradient; fold: the output
  unsigned char* b;  // compress: the residual; fold: null
  uint32_t seg;      // the segment (TopKSeg)
  uint32_t e0;       // the tile's first element in its segment
  uint32_t count;    // elements, 1..kTopKTile
  uint32_t flags;    // kTopKVec: a and b 16-byte aligned; kTopKAligned: 4-byte aligned
};
static_assert(sizeof(TopKRec) == 32, "TopKRec layout");

// One segment: compress — its payload and its tiles, records [rec_begin,
// rec_begin + nrecs); fold — `payload` unused, its sources are row `seg` of
// TopKFold::srcs.
struct TopKSeg {
  unsigned char* payload;
  uint64_t nelem;
  uint32_t k;
  uint32_t rec_begin, nrecs;
  uint32_t pad;
};
static_assert(sizeof(TopKSeg) == 32, "TopKSeg layout");

// What PICK leaves a segment: the key's digits decided so far and how many
// elements are still wanted among the keys that carry them.  After PICK 2:
// T and need_eq = k - #{key > T}.
struct TopKPick {
  uint32_t prefix, need;
};
// A tile's #{key > T}, #{key == T} (COUNT), then those of the segment's
// earlier tiles (SCAN).
struct TopKCount {
  uint32_t gt, eq;
};

struct TopKCompress {
  const TopKRec* recs;
  const TopKSeg* segs;
  uint32_t* hist;     // [nsegs * kTopKBins], zeroed by ZERO
  TopKPick* pick;     // [nsegs]
  TopKCount* count;   // [nrecs]
  TopKCount* before;  // [nrecs]
  uint32_t nrecs, nsegs;
};

struct TopKFold {
  const TopKRec* recs;
  const TopKSeg* segs;
  const unsigned char* const* srcs;  // [nsegs * nsrc] payloads, a segment's row in argument order
  uint32_t nrecs;
  int nsrc;
  int divisor;
};

// The server round: a compress whose records name the
// server's residual twice (a == b) and whose gradient is the sparse sum of row
// `seg` of `srcs`, formed in LDS by the first pass and never written.
struct TopKRefold {
  TopKCompress c;
  const unsigned char* const* srcs;  // [nsegs * nsrc] payloads, a segment's row in argument order
  int nsrc;
};

// The ten launches on `s`; `resid_bytes`: what ACCUMULATE writes (store policy).
hipError_t launch_topk_compress(const TopKCompress& p, uint64_t resid_bytes, const Tuning& tu,
                                hipStream_t s);
// The same ten with REFOLD-ACCUMULATE (bpsr_k_topk_refold.hip) in ACCUMULATE's place.
hipError_t launch_topk_refold(const TopKRefold& p, uint64_t resid_bytes, const Tuning& tu,
                              hipStream_t s);
// That one launch alone, p.c.nrecs > 0; `pol`: kPolWt or kPolNt.
hipError_t launch_topk_refold_accum(const TopKRefold& p, int pol, hipStream_t s);
// The fold; `out_bytes`: what it writes (store policy).
hipError_t launch_topk_fold(const TopKFold& p, uint64_t out_bytes, const Tuning& tu,
                            hipStream_t s);

}  // namespace bpsr
