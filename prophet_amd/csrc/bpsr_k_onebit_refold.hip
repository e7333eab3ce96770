// The server round of 1-bit sign compression: REFOLD-ACCUMULATE, the first pass
// of a compress whose input is the f32 left fold of N decoded payloads
// (prophet_amd/onebit.py's refold):
//
//   sum = ((d_0 + d_1) + ...) + d_{N-1}, d_k = +-scale_k    the fold, in registers
//   c   = sum + r over r, one f64 partial of sum |c| per wave  ACCUMULATE
//
// FINISH and PACK of bpsr_k_onebit.hip run after it unchanged, over the same
// table and the same partials: the fold's f32 output never reaches memory.
//
// The split.  A workgroup takes one compress tile (4,096 elements, 64 words);
// wave w owns words 16 w .. 16 w + 15 of it, 1,024 elements, as four chunks of
// 256: in chunk c lane l holds elements 256 c + 4 l .. + 3, one b128 of the
// residual.  Lanes 0..15 load the wave's 16 words of a source (128 contiguous
// bytes); for chunk c lane l takes word 4 c + l / 16 from the lane that holds
// it (ds_bpermute) and bits 4 (l % 16) .. + 3 of it.  16 accumulators a lane.
// The four residual loads are issued ahead of the source loop, and source
// k + 1's word and scale are in flight while source k is decoded.
//
// No LDS, no atomics; every store is a vector store.
#include "bpsr_cast_plan.h"
#include "bpsr_onebit.h"

namespace bpsr {

namespace {

constexpr int kLdAux = 2;  // streaming loads: nt
template <int POL>
constexpr int kStAux = POL == kPolWt ? 16 : 2;  // stores: sc1 (write-through) or nt
constexpr uint32_t kTileBytes = kOneBitTile * 4;
constexpr uint32_t kWaveElems = kOneBitTile / kOneBitWaves;  // 1,024: 16 words
constexpr int kChunks = 4;                                   // of 256 elements
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// The sum over the wave's 64 lanes, in every lane (bpsr_k_onebit.hip's pairing).
__device__ __forceinline__ void wave_sum(double& x) {
  const int l = (int)(threadIdx.x & 63);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1)
    x += bitcast<double>(stat_from_lane(bitcast<uint64_t>(x), (l ^ m) * 4));
}

// One source into the lane's 16 accumulators: `w` is the lane's word (lanes
// 0..15), `sb` the source's scale as bits.  FIRST: the fold starts here (no
// 0 + d: a one-source round of -0.0 stays -0.0).
template <bool FIRST>
__device__ __forceinline__ void refold_source(float (&acc)[kChunks][4], uint64_t w, uint32_t sb,
                                              uint32_t l) {
  const int lo = (int)(uint32_t)w, hi = (int)(uint32_t)(w >> 32);
#pragma unroll
  for (int c = 0; c < kChunks; ++c) {
    const int from = (4 * c + (int)(l >> 4)) * 4;
    const uint32_t tlo = (uint32_t)__builtin_amdgcn_ds_bpermute(from, lo);
    const uint32_t thi = (uint32_t)__builtin_amdgcn_ds_bpermute(from, hi);
    const uint32_t nib = ((l & 8) ? thi : tlo) >> ((l & 7) * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = bitcast<float>(sb ^ ((nib << (31 - j)) & 0x80000000u));
      acc[c][j] = FIRST ? d : acc[c][j] + d;
    }
  }
}

// c = sum + r as bits, |c| added to the lane's partial.
__device__ __forceinline__ uint32_t refold_elem(float sum, uint32_t r, double& tot) {
  const float c = sum + bitcast<float>(r);
  tot += (double)__builtin_fabsf(c);
  return bitcast<uint32_t>(c);
}

}  // namespace

template <int POL>
__global__ __launch_bounds__(kBlock) void onebit_refold_kernel(OneBitRefold p) {
  // grid == nrecs: no bounds test in front of the record load
  const OneBitRec& r = p.c.recs[blockIdx.x];
  unsigned char* const q = r.b;
  const uint32_t word0 = r.word0, count = r.count, flags = r.flags;
  const unsigned char* const* const row = p.srcs + (uint64_t)r.seg * (uint32_t)p.nsrc;
  asm volatile("" ::"s"(q), "s"(word0), "s"(count), "s"(flags), "s"(row));
  const uint32_t l = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t e0 = wave * kWaveElems;  // the wave's first element of the tile
  const bool fast = (flags & kOneBitVec) && count == kOneBitTile;
  const auto rq = __builtin_amdgcn_make_buffer_rsrc(q, 0, kTileBytes, 0x00020000);
  vec16 y[kChunks];
  if (fast) {
#pragma unroll
    for (int c = 0; c < kChunks; ++c)
      y[c] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(
          rq, (int)(e0 + (uint32_t)c * 256 + l * 4) * 4, 0, kLdAux));
  }
  // sizes come from the plan, never from a header: the wave's word l exists
  // iff it lies inside the tile's words; an absent word counts as 0
  const uint32_t nwords = (count + 63) / 64;
  const bool have = l < 16 && wave * 16 + l < nwords;
  auto load = [&](int k, uint32_t* sb) -> uint64_t {
    const unsigned char* const pl = row[k];
    *sb = *reinterpret_cast<const uint32_t*>(pl);
    if (!have) return 0;
    return __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(pl + kOneBitHeader) +
                                      word0 + wave * 16 + l);
  };
  float acc[kChunks][4];
  uint32_t sb, sn = 0;
  uint64_t w = load(0, &sb), wn = 0;
  if (p.nsrc > 1) wn = load(1, &sn);
  refold_source<true>(acc, w, sb, l);
  for (int k = 1; k < p.nsrc; ++k) {
    w = wn;
    sb = sn;
    if (k + 1 < p.nsrc) wn = load(k + 1, &sn);
    refold_source<false>(acc, w, sb, l);
  }
  double tot = 0.0;
  if (fast) {
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
#pragma unroll
      for (int j = 0; j < 4; ++j) y[c].w[j] = refold_elem(acc[c][j], y[c].w[j], tot);
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(y[c]), rq,
                                             (int)(e0 + (uint32_t)c * 256 + l * 4) * 4, 0,
                                             kStAux<POL>);
    }
  } else {
    // a ragged or misaligned tile: whole vectors where the residual is 16-byte
    // aligned and the vector inside the tile, else elements under a bounds
    // test (byte-wise where it is not 4-byte aligned); an element past count
    // is neither read nor written
    const bool vec = (flags & kOneBitVec) != 0, al = (flags & kOneBitAligned) != 0;
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
      const uint32_t e = e0 + (uint32_t)c * 256 + l * 4;
      if (vec && e + 4 <= count) {
        vec16 x = ld16<true>(q + (uint64_t)e * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) x.w[j] = refold_elem(acc[c][j], x.w[j], tot);
        st16<false>(q + (uint64_t)e * 4, x);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (e + j < count)
            st_e<uint32_t>(q + (uint64_t)(e + j) * 4,
                           refold_elem(acc[c][j], ld_e<uint32_t>(q + (uint64_t)(e + j) * 4, al),
                                       tot),
                           al);
      }
    }
  }
  // every lane is back here; a lane that read nothing adds 0
  wave_sum(tot);
  if (l == 0) p.c.part[(uint64_t)blockIdx.x * kOneBitWaves + wave] = tot;
}

hipError_t launch_onebit_refold(const OneBitRefold& p, uint64_t resid_bytes, const Tuning& tu,
                                hipStream_t s) {
  if (p.c.nsegs == 0) return hipSuccess;
  const int pol = cast_store_pol(tu, resid_bytes);
  if (p.c.nrecs) {
    const hipError_t e =
        pol == kPolWt ? launch_cast_kernel<onebit_refold_kernel<kPolWt>>(
                            p, p.c.nrecs, tu.occ_min_tiles_batch, tu, s)
                      : launch_cast_kernel<onebit_refold_kernel<kPolNt>>(
                            p, p.c.nrecs, tu.occ_min_tiles_batch, tu, s);
    if (e != hipSuccess) return e;
  }
  return launch_onebit_finish_pack(p.c, resid_bytes, tu, s);
}

}  // namespace bpsr
