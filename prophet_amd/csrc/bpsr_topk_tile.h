// Top-k sparsification: what the kernels of bpsr_k_topk.hip and of
// bpsr_k_topk_refold.hip share — the tile's lane
// map and its loads, the LDS histograms, the wave scan, and the sparse sum of a
// tile's sources in LDS: the lockstep searches and the adds in argument order.
//
// The lane map is the cast tiles': a workgroup owns 4,096 contiguous elements,
// lane l's j-th b128 vector is vector j * 256 + l, so word [j][e] of a lane is
// element 4 (256 j + l) + e of the tile and ascending element order is (j,
// wave, lane, e).
#pragma once

#include "bpsr_cast_plan.h"
#include "bpsr_topk.h"

namespace bpsr {

namespace {

constexpr int kLdAux = 2;  // streaming loads: nt
template <int POL>
constexpr int kStAux = POL == kPolWt ? 16 : 2;  // stores: sc1 (write-through) or nt
constexpr uint32_t kTileBytes = kTopKTile * 4;
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kKeyMask = 0x7fffffffu;
// digit d of a key, the bits above it, its bins and its place in a segment's histograms
constexpr uint32_t kDigitShift[3] = {kTopKBits1 + kTopKBits2, kTopKBits2, 0};
constexpr uint32_t kDigitBins[3] = {1u << kTopKBits0, 1u << kTopKBits1, 1u << kTopKBits2};
constexpr uint32_t kDigitAt[3] = {0, 1u << kTopKBits0, (1u << kTopKBits0) + (1u << kTopKBits1)};

__device__ __forceinline__ uint32_t vector_of(int j, uint32_t lane) {
  return (uint32_t)j * kBlock + lane;
}

// The lane's 16 words of the tile at `q` (count elements): the bits of those
// inside the tile set in the result, bit 4 j + e.  A whole aligned tile is
// four b128 loads issued together; anything else goes vector by vector, whole
// vectors as b128 where the operands allow, the rest element by element.
// AUX: the loads' cache policy (0, or kLdAux for a tile read once).
template <int AUX = 0>
__device__ __forceinline__ uint32_t load_tile(const unsigned char* q, uint32_t count,
                                              uint32_t flags, uint32_t lane,
                                              uint32_t (&c)[4][4]) {
  if ((flags & kTopKVec) && count == kTopKTile) {
    const auto rq = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(q), 0,
                                                      kTileBytes, 0x00020000);
    vec16 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      x[j] = bitcast<vec16>(
          __builtin_amdgcn_raw_buffer_load_b128(rq, (int)vector_of(j, lane) * 16, 0, AUX));
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) c[j][e] = x[j].w[e];
    return 0xffffu;
  }
  const bool vec = (flags & kTopKVec) != 0, al = (flags & kTopKAligned) != 0;
  uint32_t valid = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t p0 = vector_of(j, lane) * 4;
    if (vec && p0 + 4 <= count) {
      const vec16 x = ld16<AUX != 0>(q + (uint64_t)p0 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) c[j][e] = x.w[e];
      valid |= 0xfu << (4 * j);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        c[j][e] = 0;
        if (p0 + e < count) {
          c[j][e] = ld_e<uint32_t>(q + (uint64_t)(p0 + e) * 4, al);
          valid |= 1u << (4 * j + e);
        }
      }
    }
  }
  return valid;
}

// One vector's bins into the LDS histogram: the elements of mask `m` (4
// bits), equal bins of the lane added once.
__device__ __forceinline__ void hist_vector(uint32_t* h, const uint32_t (&b)[4], uint32_t m) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (!((m >> e) & 1)) continue;
    bool first = true;
#pragma unroll
    for (int d = 0; d < e; ++d) first = first && !(((m >> d) & 1) && b[d] == b[e]);
    if (!first) continue;
    uint32_t n = 1;
#pragma unroll
    for (int d = e + 1; d < 4; ++d) n += (((m >> d) & 1) && b[d] == b[e]) ? 1u : 0u;
    atomicAdd(&h[b[e]], n);
  }
}

// The workgroup's non-zero bins into the segment's histogram.
template <uint32_t BINS>
__device__ __forceinline__ void hist_flush(const uint32_t* h, uint32_t* gh) {
  for (uint32_t i = threadIdx.x; i < BINS; i += kBlock) {
    const uint32_t v = h[i];
    if (v) (void)__hip_atomic_fetch_add(gh + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The inclusive sum over the lanes up to this one (Hillis-Steele, all 64
// lanes active).
__device__ __forceinline__ uint32_t wave_scan(uint32_t x) {
  const int l = (int)(threadIdx.x & 63);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const uint32_t y = (uint32_t)__builtin_amdgcn_ds_bpermute((l - m) * 4, (int)x);
    x += l >= m ? y : 0u;
  }
  return x;
}

// The sparse sum of a tile's sources, first half: the two bounds of each
// source's index range inside [t0, t0 + count) into bound[s][0..1].  Search
// w + 4 i of the 2 nsrc is wave w's: source (w >> 1) + 2 i, the range's begin
// (w even: the entries below t0) or its end (below t0 + count).  A step probes
// 64 split points (one load a lane, one ballot) and keeps one 64th of the
// range; the searches of a wave run in lockstep.  [lo, hi] holds the answer and
// never leaves [0, k], whatever the entries are.  idx_of(s): the k indices of
// source s.  The caller's barrier comes after.
template <class IdxOf>
__device__ __forceinline__ void tile_bounds(IdxOf&& idx_of, int nsrc, uint32_t k, uint32_t t0,
                                            uint32_t count, uint32_t l, uint32_t w,
                                            uint32_t (&bound)[kTopKMaxSrcs][2]) {
  constexpr int kPerWave = 2 * kTopKMaxSrcs / (int)kTopKWaves;
  const uint32_t target = t0 + ((w & 1) ? count : 0u);
  uint32_t lo[kPerWave], hi[kPerWave];
#pragma unroll
  for (int i = 0; i < kPerWave; ++i) {
    lo[i] = 0;
    hi[i] = (int)(w >> 1) + 2 * i < nsrc ? k : 0u;
  }
  for (;;) {
    bool more = false;
    uint32_t v[kPerWave], stride[kPerWave];
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {
      const uint32_t len = hi[i] - lo[i];
      stride[i] = (len + 63) / 64;
      const uint64_t at = (uint64_t)lo[i] + (uint64_t)l * stride[i];
      v[i] = 0xffffffffu;
      if (len && at < hi[i]) v[i] = idx_of((int)(w >> 1) + 2 * i)[at];
      more = more || len;
    }
    if (!more) break;
#pragma unroll
    for (int i = 0; i < kPerWave; ++i) {
      if (hi[i] == lo[i]) continue;
      const uint64_t at = (uint64_t)lo[i] + (uint64_t)l * stride[i];
      const uint32_t below =
          (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(at < hi[i] && v[i] < target));
      if (below == 0) {
        hi[i] = lo[i];
      } else {
        const uint64_t end = (uint64_t)lo[i] + (uint64_t)below * stride[i];
        lo[i] = lo[i] + (below - 1) * stride[i] + 1;
        hi[i] = end < hi[i] ? (uint32_t)end : hi[i];
      }
    }
  }
  if (l == 0) {
#pragma unroll
    for (int i = 0; i < kPerWave; ++i)
      if ((int)(w >> 1) + 2 * i < nsrc) bound[(w >> 1) + 2 * i][w & 1] = lo[i];
  }
}

// Second half, behind that barrier: source after source, in argument order and
// a barrier apart, lanes stride the source's range and add into `tile`; the
// next source's entries are loaded ahead of this one's adds.  The guard keeps
// every write inside the tile: idx - t0 wraps far past count.  Ends on a
// barrier.
template <class IdxOf>
__device__ __forceinline__ void tile_adds(IdxOf&& idx_of, int nsrc, uint32_t k, uint32_t t0,
                                          uint32_t count, uint32_t tid,
                                          const uint32_t (&bound)[kTopKMaxSrcs][2],
                                          float (&tile)[kTopKTile]) {
  // entry `begin + tid` of source s, where the range has one
  auto fetch = [&](int s, uint32_t* ii, float* vv) {
    const uint32_t at = bound[s][0] + tid;
    *ii = 0xffffffffu;
    *vv = 0.0f;
    if (at < bound[s][1]) {
      *ii = idx_of(s)[at];
      *vv = reinterpret_cast<const float*>(idx_of(s) + k)[at];
    }
  };
  uint32_t ci, ni = 0xffffffffu;
  float cv, nv = 0.0f;
  fetch(0, &ci, &cv);
  for (int s = 0; s < nsrc; ++s) {
    if (s + 1 < nsrc) fetch(s + 1, &ni, &nv);
    if (ci - t0 < count) tile[ci - t0] = tile[ci - t0] + cv;
    const uint32_t end = bound[s][1];
    for (uint64_t at = (uint64_t)bound[s][0] + tid + kBlock; at < end; at += kBlock) {
      const uint32_t ii = idx_of(s)[at];
      const float vv = reinterpret_cast<const float*>(idx_of(s) + k)[at];
      if (ii - t0 < count) tile[ii - t0] = tile[ii - t0] + vv;
    }
    __syncthreads();
    ci = ni;
    cv = nv;
  }
}

}  // namespace

}  // namespace bpsr
