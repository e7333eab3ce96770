// Block-scaled 8- and 4-bit wires with error feedback (byteps_reduce_mx_*,
// DESIGN.md §11.13; the definition is prophet_amd/mx.py).  What the host side
// (bpsr_mx.cpp: operand checks, tables, the C entry points) and the kernels
// (bpsr_k_mx.hip) share: the payload's layout, the tables' records and the
// launches.
//
// A payload is a 16-byte header {u32 bits, u32 n_lo, u32 n_hi, u32 0}, one E8M0
// scale byte a block of 32 elements, padded with zeros to 16 bytes, and the
// element codes — OCP e4m3 bytes or OCP e2m1 nibbles, element 2 j in the low
// one — padded with zeros to 16 bytes.
//
// A compress is one launch over a table of tiles, a fold is one launch over a
// table of output tiles; neither has scratch memory.
#pragma once

#include "bpsr_internal.h"

namespace bpsr {

constexpr uint64_t kMxHeader = 16;
constexpr uint32_t kMxBlock = 32;
// A tile: kBlock lanes x 4 b128 vectors, 4,096 elements a workgroup; vector
// j * kBlock + lane is lane's j-th, so a block is eight adjacent lanes of one j
// and a tile holds 128 blocks.  Tiles start on multiples of the tile in their
// segment: on block boundaries, and 16-byte aligned in the scales and the codes.
constexpr uint32_t kMxTile = kBlock * 16;
constexpr uint32_t kMxTileBlocks = kMxTile / kMxBlock;
constexpr int kMxMaxSrcs = 16;
constexpr uint64_t kMxMaxElems = 1ull << 31;

constexpr uint64_t mx_align16(uint64_t x) { return (x + 15) & ~15ull; }
constexpr uint64_t mx_scale_bytes(uint64_t n) { return (n + kMxBlock - 1) / kMxBlock; }
constexpr uint64_t mx_code_bytes(uint64_t n, uint32_t bits) { return (n * bits + 7) / 8; }
// where the codes begin in a payload of n elements
constexpr uint64_t mx_codes_at(uint64_t n) { return kMxHeader + mx_align16(mx_scale_bytes(n)); }
constexpr uint64_t mx_payload_bytes(uint64_t n, uint32_t bits) {
  return mx_codes_at(n) + mx_align16(mx_code_bytes(n, bits));
}

// One tile of a compress or of a fold: both pointers already advanced to the
// tile's first element.  A compress of an empty segment that names a payload
// is one record of count 0: it writes the header.
enum : uint32_t { kMxVec = 1, kMxAligned = 2, kMxVecB = 4 };
struct MxRec {
  unsigned char* a;  // compress: the gradient; fold: the output; refold: the residual
  unsigned char* b;  // compress: the residual; fold, refold: null
  uint32_t seg;      // the segment (MxSeg)
  uint32_t e0;       // the tile's first element in its segment
  uint32_t count;    // elements, 0..kMxTile
  // f32 plans — kMxVec: a and b 16-byte aligned; kMxAligned: 4-byte aligned.
  // 2-byte plans — kMxVec: a 16-byte aligned; kMxVecB: b 16-byte aligned (an
  // operand is always aligned to its element there).
  uint32_t flags;
};
static_assert(sizeof(MxRec) == 32, "MxRec layout");

// One segment: compress — its payload; fold — `payload` unused, its sources
// are row `seg` of MxFold::srcs.
struct MxSeg {
  unsigned char* payload;
  uint64_t nelem;
};
static_assert(sizeof(MxSeg) == 16, "MxSeg layout");

struct MxCompress {
  const MxRec* recs;
  const MxSeg* segs;
  uint32_t nrecs;
};

struct MxFold {
  const MxRec* recs;
  const MxSeg* segs;
  const unsigned char* const* srcs;  // [nsegs * nsrc] payloads, a segment's row in argument order
  uint32_t nrecs;
  int nsrc;
  int divisor;
};

// `bits`: 8 or 4.  `resid_bytes` / `out_bytes`: what the launch writes in f32
// (store policy).
hipError_t launch_mx_compress(const MxCompress& p, uint32_t bits, uint64_t resid_bytes,
                              const Tuning& tu, hipStream_t s);
hipError_t launch_mx_fold(const MxFold& p, uint32_t bits, uint64_t out_bytes, const Tuning& tu,
                          hipStream_t s);

// The server round (byteps_reduce_mx_refold_*; the kernel is
// bpsr_k_mx_refold.hip): the fold's sum plus the residual, compressed, in one
// launch.  Records are MxRec with `a` the residual's tile and `b` null; a
// segment's `payload` is the one written, its sources row `seg` of `srcs`.  An
// empty segment that names an output payload is one record of count 0.
struct MxRefold {
  const MxRec* recs;
  const MxSeg* segs;
  const unsigned char* const* srcs;  // as MxFold::srcs
  uint32_t nrecs;
  int nsrc;
};

hipError_t launch_mx_refold(const MxRefold& p, uint32_t bits, uint64_t resid_bytes,
                            const Tuning& tu, hipStream_t s);

// The stateless wires (byteps_reduce_mx_sr_*, byteps_reduce_mx_rht_fold_*,
// DESIGN.md §11.15; the definition is prophet_amd/mx_sr.py; the kernels are
// bpsr_k_mx_sr.hip).  Records are MxRec with `b` null; a segment carries the key
// its elements round under and the key its whole blocks are rotated under.
struct MxSrSeg {
  unsigned char* payload;  // compress; unused by the rotated fold
  uint64_t nelem;
  uint32_t key, rot_key;
  uint32_t pad[2];
};
static_assert(sizeof(MxSrSeg) == 32, "MxSrSeg layout");

struct MxSrCompress {
  const MxRec* recs;
  const MxSrSeg* segs;
  uint32_t nrecs;
  uint32_t step;
};

struct MxRhtFold {
  const MxRec* recs;
  const MxSrSeg* segs;
  const unsigned char* const* srcs;  // as MxFold::srcs
  uint32_t nrecs;
  int nsrc;
  int divisor;
  uint32_t step;
};

hipError_t launch_mx_sr_compress(const MxSrCompress& p, uint32_t bits, bool rotate,
                                 hipStream_t s);
hipError_t launch_mx_rht_fold(const MxRhtFold& p, uint32_t bits, uint64_t out_bytes,
                              const Tuning& tu, hipStream_t s);

// The same four launches over 2-byte tensors (the kernels are
// bpsr_k_mx_half.hip): `dtype` is kFloat16 or kBFloat16, the type of MxRec::a —
// the gradient of a compress, the output of a fold.  MxRec::b, the residual,
// stays f32; `resid_bytes` / `out_bytes` are what the launch writes.
hipError_t launch_mx_half_compress(const MxCompress& p, int dtype, uint32_t bits,
                                   uint64_t resid_bytes, const Tuning& tu, hipStream_t s);
hipError_t launch_mx_half_sr_compress(const MxSrCompress& p, int dtype, uint32_t bits,
                                      bool rotate, hipStream_t s);
hipError_t launch_mx_half_fold(const MxFold& p, int dtype, uint32_t bits, uint64_t out_bytes,
                               const Tuning& tu, hipStream_t s);
hipError_t launch_mx_half_rht_fold(const MxRhtFold& p, int dtype, uint32_t bits,
                                   uint64_t out_bytes, const Tuning& tu, hipStream_t s);

}  // namespace bpsr
