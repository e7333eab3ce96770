// The server round of the top-k wire (topk_ef; the definition
// is prophet_amd/topk.py's refold = compress(fold(payloads, n, 1, k), r, k)):
//
//   REFOLD-ACCUMULATE  c = (+0 + s_0 + ... + s_{N-1}) + r over r, the sparse sum
//                      in LDS; histogram of key >> 20 (11 bits)
//
// It stands where ACCUMULATE stands in the compress's ten launches
// (bpsr_k_topk.hip, launch_topk_refold) and leaves what ACCUMULATE leaves — c
// over the residual, digit 0's histogram — so PICK, REFINE, COUNT, SCAN and
// COMPACT run unchanged behind it.  The dense sum never reaches memory.
//
// One workgroup a tile record of 4,096 elements, the compress's lane map.
// Order of the work in a tile:
//
//   1. the residual's four b128 nt loads go out; their 16 VGPRs are first read
//      in step 5.  They depend on nothing and are in flight under steps 2-3;
//   2. the 16 KiB sum tile and the 8 KiB histogram are zeroed in LDS;
//   3. the 2 N bounds of the sources' index ranges inside the tile: the
//      lockstep 64-way searches of bpsr_topk_tile.h.  A wave's number goes
//      through readfirstlane and the row of source pointers through the
//      constant address space, so the pointers arrive by scalar loads and no
//      probe waits on a vector load of its own address;
//   4. source after source in argument order, a barrier apart, the sparse adds
//      into LDS, the next source's entries fetched ahead of this one's adds;
//   5. each lane reads its four vectors of the sum as b128, c = sum + r (one
//      IEEE add, the sum first: the definition's g + r), c stored over r under
//      the store policy, the key's top digit into the LDS histogram;
//   6. the non-zero bins flushed with global integer atomics.
//
// Sizes come from the plan, never from a header.  A malformed payload gives
// wrong values; an LDS write happens only under idx - e0 < count and a search
// never leaves [0, k], so nothing is written outside the tile and nothing read
// outside a payload's 16 + 8 k bytes.  Ragged last tiles and a residual 4 bytes
// off a 16-byte boundary take load_tile's per-vector and per-element paths and
// the matching stores; an element past count is neither read nor written.
#include "bpsr_topk_tile.h"

namespace bpsr {

template <int POL>
__global__ __launch_bounds__(kBlock) void topk_refold_accum_kernel(TopKRefold p) {
  __shared__ __attribute__((aligned(16))) float tile[kTopKTile];
  __shared__ __attribute__((aligned(16))) uint32_t h[kDigitBins[0]];
  __shared__ uint32_t bound[kTopKMaxSrcs][2];
  // grid == nrecs: no bounds test in front of the record load
  const TopKRec& r = p.c.recs[blockIdx.x];
  unsigned char* const q = r.b;
  const uint32_t seg = r.seg, e0 = r.e0, count = r.count, flags = r.flags;
  const uint32_t k = p.c.segs[seg].k;
  const int nsrc = p.nsrc;
  asm volatile("" ::"s"(q), "s"(seg), "s"(e0), "s"(count), "s"(flags), "s"(k), "s"(nsrc));
  // read-only for the launch: through the constant address space a uniform
  // index gives a scalar load
  typedef const unsigned char* SrcPtr;
  const auto* const row = (const __attribute__((address_space(4))) SrcPtr*)(
      p.srcs + (uint64_t)seg * (uint32_t)nsrc);
  auto idx_of = [&](int s) { return reinterpret_cast<const uint32_t*>(row[s] + kTopKHeader); };
  const uint32_t tid = threadIdx.x, l = tid & 63;
  const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));

  // the residual: issued here, first used after the last source's adds
  uint32_t c[4][4];
  const uint32_t valid = load_tile<kLdAux>(q, count, flags, tid, c);

#pragma unroll
  for (int j = 0; j < 4; ++j)
    *reinterpret_cast<u4*>(&tile[vector_of(j, tid) * 4]) = u4{0, 0, 0, 0};
#pragma unroll
  for (uint32_t i = 0; i < kDigitBins[0] / (4 * kBlock); ++i)
    *reinterpret_cast<u4*>(&h[(i * kBlock + tid) * 4]) = u4{0, 0, 0, 0};

  tile_bounds(idx_of, nsrc, k, e0, count, l, w, bound);
  __syncthreads();  // the bounds, and both zeroings
  tile_adds(idx_of, nsrc, k, e0, count, tid, bound, tile);

  const bool vec = (flags & kTopKVec) != 0, al = (flags & kTopKAligned) != 0;
  const bool full = vec && count == kTopKTile;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t p0 = vector_of(j, tid) * 4;
    // past count the tile holds +0.0 and c is 0: nothing of it is stored or counted
    const vec16 sum = bitcast<vec16>(*reinterpret_cast<const u4*>(&tile[p0]));
    vec16 y;
    uint32_t b[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      y.w[e] = bitcast<uint32_t>(bitcast<float>(sum.w[e]) + bitcast<float>(c[j][e]));
      b[e] = (y.w[e] & kKeyMask) >> kDigitShift[0];
    }
    if (full) {
      const auto rq = __builtin_amdgcn_make_buffer_rsrc(q, 0, kTileBytes, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(y), rq, (int)p0 * 4, 0, kStAux<POL>);
    } else if (vec && p0 + 4 <= count) {
      st16<false>(q + (uint64_t)p0 * 4, y);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((valid >> (4 * j + e)) & 1) st_e<uint32_t>(q + (uint64_t)(p0 + e) * 4, y.w[e], al);
    }
    hist_vector(h, b, (valid >> (4 * j)) & 0xfu);
  }
  __syncthreads();
  hist_flush<kDigitBins[0]>(h, p.c.hist + (uint64_t)seg * kTopKBins);
}

hipError_t launch_topk_refold_accum(const TopKRefold& p, int pol, hipStream_t s) {
  // static LDS: a plain launch, no residency request on top
  if (pol == kPolWt)
    hipLaunchKernelGGL(topk_refold_accum_kernel<kPolWt>, dim3(p.c.nrecs), dim3(kBlock), 0, s, p);
  else
    hipLaunchKernelGGL(topk_refold_accum_kernel<kPolNt>, dim3(p.c.nrecs), dim3(kBlock), 0, s, p);
  return hipGetLastError();
}

}  // namespace bpsr
