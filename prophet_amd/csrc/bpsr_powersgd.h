// PowerSGD low-rank compression with error feedback (byteps_reduce_powersgd_*,
// DESIGN.md §11.14; the definition is prophet_amd/powersgd.py).  What the host
// side (bpsr_powersgd.cpp: operand checks, tables, the C entry points) and the
// kernels (bpsr_k_powersgd.hip) share: the segment record, the work records of
// the three tiled phases, the rules that cut a matrix into chunks, and the
// launches.
//
// A segment is one row-major n x m float32 matrix M with its rank r: g, R and
// out are n x m, P is n x r, Q and Qn are m x r.  A phase is a fixed sequence
// of launches on one stream; no workgroup waits on another and nothing is
// added with atomics: every projection writes per-chunk partial tiles into
// the plan's scratch, and REDUCE adds a segment's chunks up in chunk order.
#pragma once

#include "bpsr_internal.h"

namespace bpsr {

constexpr uint32_t kPsgdMaxRank = 16;    // the MFMA tile's N
constexpr uint64_t kPsgdMaxDim = 1ull << 24;
constexpr uint64_t kPsgdMaxElems = 1ull << 33;

// PROJECT-P: a workgroup owns kPsgdPRows rows (16 a wave) and one chunk of
// columns, a multiple of kPsgdKStep and at most kPsgdKcMax (the chunk's Q rows
// sit in LDS in operand order: 16 floats a column).
constexpr uint32_t kPsgdPRows = 64, kPsgdKStep = 64, kPsgdKcMax = 512;
// PROJECT-Q: a workgroup owns kPsgdQCols columns (64 a wave) and one chunk of
// rows, a multiple of kPsgdRStep.
constexpr uint32_t kPsgdQCols = 256, kPsgdRStep = 32;
// FINISH: a tile of kPsgdFRows rows by kPsgdFCols columns.
constexpr uint32_t kPsgdFRows = 32, kPsgdFCols = 256;
// Workgroups a projection of one segment is cut for, where the matrix allows.
constexpr uint32_t kPsgdWantGroups = 1024;

constexpr uint32_t psgd_ceil(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }
constexpr uint32_t psgd_round(uint64_t a, uint64_t b) { return psgd_ceil(a, b) * (uint32_t)b; }

// The column chunk of PROJECT-P.  A chunk costs 8 r bytes of partials a row
// against 12 bytes an element of the sweep: chunks of 6 r columns or more keep
// the partials under an eighth of it.
constexpr uint32_t psgd_kc(uint64_t n, uint64_t m, uint32_t r) {
  const uint32_t want = kPsgdWantGroups / psgd_ceil(n, kPsgdPRows);
  const uint32_t most = psgd_ceil(m, psgd_round(6 * r, kPsgdKStep));
  const uint32_t chunks = most < want ? most : (want ? want : 1);
  const uint32_t kc = psgd_round(psgd_ceil(m, chunks), kPsgdKStep);
  return kc < kPsgdKcMax ? kc : kPsgdKcMax;
}
// The row chunk of PROJECT-Q: 8 r bytes of partials a column against 4 bytes an
// element, so chunks of 16 r rows or more.
constexpr uint32_t psgd_rc(uint64_t n, uint64_t m, uint32_t r) {
  const uint32_t want = kPsgdWantGroups / psgd_ceil(m, kPsgdQCols);
  const uint32_t most = psgd_ceil(n, psgd_round(16 * r, kPsgdRStep));
  const uint32_t chunks = most < want ? most : (want ? want : 1);
  return psgd_round(psgd_ceil(n, chunks), kPsgdRStep);
}
// float32 elements of one segment's partials: the larger of the two projections'.
constexpr uint64_t psgd_scratch_elems(uint64_t n, uint64_t m, uint32_t r) {
  const uint64_t p = (uint64_t)psgd_ceil(m, psgd_kc(n, m, r)) * n * r;
  const uint64_t q = (uint64_t)psgd_ceil(n, psgd_rc(n, m, r)) * m * r;
  return p > q ? p : q;
}

struct PsgdSeg {
  const float* g;
  float* R;
  float* P;
  const float* Q;  // the warm start: PROJECT-P reads it
  float* Qn;       // PROJECT-Q writes it, FINISH reads it
  float* out;
  float* scratch;  // [chunk][n][r] (PROJECT-P) or [chunk][m][r] (PROJECT-Q)
  uint32_t n, m, r;
  uint32_t kc, pchunks;  // PROJECT-P: columns a chunk, chunks
  uint32_t rc, qchunks;  // PROJECT-Q: rows a chunk, chunks
  uint32_t vec;          // m % 4 == 0: every row is 16-byte aligned
};
static_assert(sizeof(PsgdSeg) == 88, "PsgdSeg layout");

// One workgroup of a tiled phase.  PROJECT-P: a = row panel, b = column chunk;
// PROJECT-Q: a = column tile, b = row chunk; FINISH: a = row tile, b = column tile.
struct PsgdRec {
  uint32_t seg, a, b;
};

struct PsgdArgs {
  const PsgdSeg* segs;
  const PsgdRec* recs;  // of the phase
  uint32_t nrecs, nsegs;
};

hipError_t launch_psgd_project_p(const PsgdArgs& a, hipStream_t s);
hipError_t launch_psgd_project_q(const PsgdArgs& a, hipStream_t s);
hipError_t launch_psgd_finish(const PsgdArgs& a, hipStream_t s);
// `q`: the partials are PROJECT-Q's, summed into Qn; else PROJECT-P's into P.
// `most`: the largest n r (m r) of any segment.
hipError_t launch_psgd_reduce(const PsgdArgs& a, bool q, uint64_t most, hipStream_t s);
hipError_t launch_psgd_orthogonalize(const PsgdArgs& a, hipStream_t s);

}  // namespace bpsr
