// 1-bit sign compression with error feedback: the four kernels of
// bpsr_onebit.h (the arithmetic is prophet_amd/onebit.py's,
// every line one IEEE f32 operation, nothing contracted).
//
//   ACCUMULATE  c = g + r over r, one f64 partial of sum |c| per wave
//   FINISH      scale = f32(sum / n) per segment, the payload's header
//   PACK        r' = c - (c < 0 ? -scale : scale), the bit words
//   FOLD        out = ((d_0 + d_1) + ...) + d_{N-1} [/ divisor], d_k = +-scale_k
//
// The lane-to-bit map.  ACCUMULATE streams g and r as the cast kernels do
// (b128, lane + j * kBlock, every load of the tile ahead of its first use); it
// needs no bit.  PACK reads c back — one buffer, fresh in L2 — as DWORDS at a
// stride of 64: load k of a wave reads elements 64 k + l of the wave's 1,024,
// 256 contiguous bytes, so ONE ballot of (c < 0) is word k, bit for bit, with
// no interleave on either unit (DESIGN.md §11.10 has the count against the two
// b128 maps).  Lane k keeps word k, and lanes 0..15 store the wave's 16 words
// with one vector store, 128 contiguous bytes.
//
// FOLD works the other way round, on b128 stores (it writes 4 bytes an element
// and reads N / 8): a wave takes 64 words of every source, lane l loads word l
// — 512 contiguous bytes an instruction — and for output chunk c (256 elements,
// words 4 c .. 4 c + 3) lane l fetches the word of its 16-lane row from lane
// 4 c + l / 16 and takes bits 4 (l % 16) .. + 3 of it.  The fold over the
// sources runs in argument order on 64 accumulators a lane; the next source's
// word is loaded while this one is added.
//
// No LDS but FINISH's 16 wave totals, no atomics; every store is a vector store.
#include "bpsr_cast_plan.h"
#include "bpsr_onebit.h"

namespace bpsr {

namespace {

constexpr int kLdAux = 2;  // streaming loads: nt
template <int POL>
constexpr int kStAux = POL == kPolWt ? 16 : 2;  // stores: sc1 (write-through) or nt
constexpr uint32_t kTileBytes = kOneBitTile * 4;
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// The sum over the wave's 64 lanes, in every lane (stat_wave_sum's pairing).
__device__ __forceinline__ void wave_sum(double& x) {
  const int l = (int)(threadIdx.x & 63);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1)
    x += bitcast<double>(stat_from_lane(bitcast<uint64_t>(x), (l ^ m) * 4));
}

// c = g + r as bits, |c| added to the lane's partial.
__device__ __forceinline__ uint32_t accum_elem(uint32_t g, uint32_t r, double& sum) {
  const float c = bitcast<float>(g) + bitcast<float>(r);
  sum += (double)__builtin_fabsf(c);
  return bitcast<uint32_t>(c);
}

// r' of one element whose sign bit is `neg`.
__device__ __forceinline__ uint32_t pack_elem(float c, bool neg, float scale) {
  const float d = neg ? -scale : scale;
  return bitcast<uint32_t>(c - d);
}

}  // namespace

template <int POL>
__global__ __launch_bounds__(kBlock) void onebit_accum_kernel(OneBitCompress p) {
  // grid == nrecs: no bounds test in front of the record load
  const OneBitRec& r = p.recs[blockIdx.x];
  const unsigned char* const g = r.a;
  unsigned char* const q = r.b;
  const uint32_t count = r.count, flags = r.flags;
  asm volatile("" ::"s"(g), "s"(q), "s"(count), "s"(flags));
  const uint32_t lane = threadIdx.x;
  double sum = 0.0;
  if ((flags & kOneBitVec) && count == kOneBitTile) {
    const auto rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(g), 0,
                                                      kTileBytes, 0x00020000);
    const auto rq = __builtin_amdgcn_make_buffer_rsrc(q, 0, kTileBytes, 0x00020000);
    vec16 x[4], y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int off = (j * kBlock + (int)lane) * 16;
      x[j] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rg, off, 0, kLdAux));
      y[j] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rq, off, 0, kLdAux));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) y[j].w[e] = accum_elem(x[j].w[e], y[j].w[e], sum);
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(y[j]), rq, (j * kBlock + (int)lane) * 16,
                                             0, kStAux<POL>);
    }
  } else if (flags & kOneBitVec) {
    // the segment's last tile: whole vectors, then at most 3 elements
    const uint32_t nvec = count / 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t v = (uint32_t)j * kBlock + lane;
      if (v >= nvec) continue;
      const vec16 x = ld16<true>(g + (uint64_t)v * 16);
      vec16 y = ld16<true>(q + (uint64_t)v * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) y.w[e] = accum_elem(x.w[e], y.w[e], sum);
      st16<false>(q + (uint64_t)v * 16, y);
    }
    const uint32_t e = nvec * 4 + lane;
    if (e < count)
      st_e<uint32_t>(q + (uint64_t)e * 4,
                     accum_elem(ld_e<uint32_t>(g + (uint64_t)e * 4, true),
                                ld_e<uint32_t>(q + (uint64_t)e * 4, true), sum),
                     true);
  } else {
    const bool al = (flags & kOneBitAligned) != 0;
    for (uint32_t e = lane; e < count; e += kBlock)
      st_e<uint32_t>(q + (uint64_t)e * 4,
                     accum_elem(ld_e<uint32_t>(g + (uint64_t)e * 4, al),
                                ld_e<uint32_t>(q + (uint64_t)e * 4, al), sum),
                     al);
  }
  // every lane is back here; a lane that read nothing adds 0
  wave_sum(sum);
  if ((lane & 63) == 0) p.part[(uint64_t)blockIdx.x * kOneBitWaves + (lane >> 6)] = sum;
}

// One workgroup per segment, on the stream of ACCUMULATE (the kernel boundary
// makes every XCD's partials visible).  The segment's partials are contiguous
// and ascending by (tile, wave); lane t adds partials t, t + kFinishBlock, ...
// as they come, the waves add their lanes up (wave_sum) and lane 0 the waves,
// in wave order: an order the plan alone fixes.  A segment of 64 Mi elements
// has 64 Ki partials, so 1,024 lanes with four loads in flight each.
constexpr uint32_t kFinishBlock = 1024, kFinishAhead = 4;
__global__ __launch_bounds__(kFinishBlock) void onebit_finish_kernel(OneBitCompress p) {
  __shared__ double wsum[kFinishBlock / 64];
  const OneBitSeg& sg = p.segs[blockIdx.x];
  unsigned char* const payload = sg.payload;
  const uint64_t nelem = sg.nelem;
  const double* const part = p.part + (uint64_t)sg.rec_begin * kOneBitWaves;
  const uint64_t n = (uint64_t)sg.nrecs * kOneBitWaves;
  double sum = 0.0;
  for (uint64_t i0 = threadIdx.x; i0 < n; i0 += (uint64_t)kFinishBlock * kFinishAhead) {
    double x[kFinishAhead];
#pragma unroll
    for (uint32_t a = 0; a < kFinishAhead; ++a) {
      const uint64_t i = i0 + (uint64_t)a * kFinishBlock;
      x[a] = i < n ? part[i] : 0.0;
    }
#pragma unroll
    for (uint32_t a = 0; a < kFinishAhead; ++a)
      if (i0 + (uint64_t)a * kFinishBlock < n) sum += x[a];
  }
  wave_sum(sum);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0 && payload) {
    double total = wsum[0];
    for (uint32_t w = 1; w < kFinishBlock / 64; ++w) total += wsum[w];
    const float scale = nelem ? (float)(total / (double)nelem) : 0.0f;
    vec16 h;
    h.w[0] = bitcast<uint32_t>(scale);
    h.w[1] = (uint32_t)nelem;
    h.w[2] = (uint32_t)(nelem >> 32);
    h.w[3] = 0;
    st16<false>(payload, h);
  }
}

template <int POL>
__global__ __launch_bounds__(kBlock) void onebit_pack_kernel(OneBitCompress p) {
  const OneBitRec& r = p.recs[blockIdx.x];
  unsigned char* const q = r.b;
  const uint32_t seg = r.seg, word0 = r.word0, count = r.count, flags = r.flags;
  unsigned char* const payload = p.segs[seg].payload;
  // the scale FINISH left in the header: a wave-uniform load, ahead of every store
  const float scale = *reinterpret_cast<const float*>(payload);
  asm volatile("" ::"s"(q), "s"(payload), "s"(word0), "s"(count), "s"(flags));
  uint64_t* const words = reinterpret_cast<uint64_t*>(payload + kOneBitHeader) + word0;
  const uint32_t l = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t e0 = wave * (kOneBitTile / kOneBitWaves);  // the wave's 16 words
  uint64_t mine = 0;  // lane k: word k of the wave
  if ((flags & kOneBitAligned) && count == kOneBitTile) {
    const auto rq = __builtin_amdgcn_make_buffer_rsrc(q, 0, kTileBytes, 0x00020000);
    uint32_t c[16];
#pragma unroll
    for (int k = 0; k < 16; ++k)
      c[k] = __builtin_amdgcn_raw_buffer_load_b32(rq, (int)(e0 + k * 64 + l) * 4, 0, 0);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float cf = bitcast<float>(c[k]);
      const bool neg = cf < 0.0f;
      const uint64_t w = __builtin_amdgcn_ballot_w64(neg);
      __builtin_amdgcn_raw_buffer_store_b32(pack_elem(cf, neg, scale), rq,
                                            (int)(e0 + k * 64 + l) * 4, 0, kStAux<POL>);
      mine = l == (uint32_t)k ? w : mine;
    }
    if (l < 16) words[wave * 16 + l] = mine;
  } else {
    // a ragged or element-misaligned tile: an element past count is neither
    // read nor written, and its bit is 0
    const bool al = (flags & kOneBitAligned) != 0;
#pragma unroll 4
    for (uint32_t k = 0; k < 16; ++k) {
      const uint32_t e = e0 + k * 64 + l;
      const bool valid = e < count;
      float cf = 0.0f;
      if (valid) cf = bitcast<float>(ld_e<uint32_t>(q + (uint64_t)e * 4, al));
      const bool neg = valid && cf < 0.0f;
      const uint64_t w = __builtin_amdgcn_ballot_w64(neg);
      if (valid) st_e<uint32_t>(q + (uint64_t)e * 4, pack_elem(cf, neg, scale), al);
      mine = l == k ? w : mine;
    }
    const uint32_t nwords = (count + 63) / 64;
    if (l < 16 && wave * 16 + l < nwords) words[wave * 16 + l] = mine;
  }
}

// One source into the wave's 64 accumulators a lane: `w` is the lane's word,
// `sb` the source's scale as bits.  FIRST: the fold starts here (no 0 + d: a
// one-source fold of -0.0 stays -0.0).
template <bool FIRST>
__device__ __forceinline__ void fold_source(float (&acc)[16][4], uint64_t w, uint32_t sb,
                                            uint32_t l) {
  const int lo = (int)(uint32_t)w, hi = (int)(uint32_t)(w >> 32);
#pragma unroll
  for (int c = 0; c < 16; ++c) {
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

template <int POL>
__global__ __launch_bounds__(kBlock) void onebit_fold_kernel(OneBitFold p) {
  // one record a WAVE; the last workgroup's spare waves leave whole
  const uint32_t wr = (uint32_t)__builtin_amdgcn_readfirstlane(
      (int)(blockIdx.x * kOneBitWaves + (threadIdx.x >> 6)));
  if (wr >= p.nrecs) return;
  const OneBitRec& r = p.recs[wr];
  unsigned char* const out = r.a;
  const uint32_t word0 = r.word0, count = r.count, flags = r.flags;
  const unsigned char* const* const row = p.srcs + (uint64_t)r.seg * (uint32_t)p.nsrc;
  const uint32_t l = threadIdx.x & 63;
  // sizes come from the plan, never from a header: word l exists iff l < nwords
  const uint32_t nwords = (count + 63) / 64;
  auto load = [&](int k, uint32_t* sb) -> uint64_t {
    const unsigned char* const pl = row[k];
    *sb = *reinterpret_cast<const uint32_t*>(pl);
    if (l >= nwords) return 0;
    return __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(pl + kOneBitHeader) +
                                      word0 + l);
  };
  float acc[16][4];
  uint32_t sb, sn = 0;
  uint64_t w = load(0, &sb), wn = 0;
  if (p.nsrc > 1) wn = load(1, &sn);
  fold_source<true>(acc, w, sb, l);
  for (int k = 1; k < p.nsrc; ++k) {
    w = wn;
    sb = sn;
    if (k + 1 < p.nsrc) wn = load(k + 1, &sn);
    fold_source<false>(acc, w, sb, l);
  }
  if (p.divisor > 1) {
    const float fd = (float)p.divisor;
#pragma unroll
    for (int c = 0; c < 16; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[c][j] = acc[c][j] / fd;
  }
  if ((flags & kOneBitVec) && count == kOneBitTile) {
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(out, 0, kTileBytes, 0x00020000);
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      vec16 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o.w[j] = bitcast<uint32_t>(acc[c][j]);
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(o), ro, (c * 64 + (int)l) * 16, 0,
                                             kStAux<POL>);
    }
  } else {
    const bool vec = (flags & kOneBitVec) != 0, al = (flags & kOneBitAligned) != 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const uint32_t e = (uint32_t)c * 256 + l * 4;
      if (vec && e + 4 <= count) {
        vec16 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o.w[j] = bitcast<uint32_t>(acc[c][j]);
        st16<true>(out + (uint64_t)e * 4, o);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (e + j < count)
            st_e<uint32_t>(out + (uint64_t)(e + j) * 4, bitcast<uint32_t>(acc[c][j]), al);
      }
    }
  }
}

// f(POL) with the store policy as a std::integral_constant.
template <class F>
static hipError_t onebit_with_pol(int pol, F&& f) {
  return pol == kPolWt ? f(std::integral_constant<int, kPolWt>{})
                       : f(std::integral_constant<int, kPolNt>{});
}

hipError_t launch_onebit_compress(const OneBitCompress& p, uint64_t resid_bytes, const Tuning& tu,
                                  hipStream_t s) {
  if (p.nsegs == 0) return hipSuccess;
  const hipError_t e = onebit_with_pol(cast_store_pol(tu, resid_bytes), [&](auto POL) {
    if (!p.nrecs) return hipSuccess;
    return launch_cast_kernel<onebit_accum_kernel<decltype(POL)::value>>(
        p, p.nrecs, tu.occ_min_tiles_batch, tu, s);
  });
  return e == hipSuccess ? launch_onebit_finish_pack(p, resid_bytes, tu, s) : e;
}

// FINISH and PACK alone: the tail of a compress whose first pass has run on
// `s` (ACCUMULATE above, or bpsr_k_onebit_refold.hip's REFOLD-ACCUMULATE).
hipError_t launch_onebit_finish_pack(const OneBitCompress& p, uint64_t resid_bytes,
                                     const Tuning& tu, hipStream_t s) {
  if (p.nsegs == 0) return hipSuccess;
  return onebit_with_pol(cast_store_pol(tu, resid_bytes), [&](auto POL) {
    constexpr int kPol = decltype(POL)::value;
    hipLaunchKernelGGL(onebit_finish_kernel, dim3(p.nsegs), dim3(kFinishBlock), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !p.nrecs) return e;
    return launch_cast_kernel<onebit_pack_kernel<kPol>>(p, p.nrecs, tu.occ_min_tiles_batch, tu, s);
  });
}

hipError_t launch_onebit_fold(const OneBitFold& p, uint64_t out_bytes, const Tuning& tu,
                              hipStream_t s) {
  if (p.nrecs == 0) return hipSuccess;
  const uint64_t grid = ((uint64_t)p.nrecs + kOneBitWaves - 1) / kOneBitWaves;
  return onebit_with_pol(cast_store_pol(tu, out_bytes), [&](auto POL) {
    return launch_cast_kernel<onebit_fold_kernel<decltype(POL)::value>>(
        p, grid, tu.occ_min_tiles_batch, tu, s);
  });
}

}  // namespace bpsr
