// Stateless block-scaled 8- and 4-bit wires: the kernels of bpsr_mx.h's second
// half (the definition is prophet_amd/mx_sr.py).
//
//   COMPRESS  [c = H D g, whole blocks;] per block of 32 the scale byte X from
//             the largest key, bumped where 2^emax would not hold it; the codes
//             of c 2^(127 - X) rounded up with the probability of the dropped
//             fraction, under 16 Philox bits an element
//   RHT FOLD  t = d_0 + d_1 + ... + d_{N-1} in registers; out = D H t 2^-5
//             [/ divisor]
//
// Both are one launch, one workgroup a tile record, no scratch memory, no
// residual: the compress reads g and writes codes and scales.  Tile and lane
// map are bpsr_k_mx.hip's (bpsr_mx_lanes.h): word [j][e] of lane l is element
// 4 (256 j + l) + e of the tile, and a block is the j-th vectors of eight
// adjacent lanes, element 4 (l % 8) + e of the block.
//
// Rounding bits: one philox2x32_10(c0 = vector index in the tensor, c1 = step,
// k = key) a lane and j — a tile starts on a multiple of 4,096 elements, so
// the vector is one Philox group of bpsr_cast_sr.h.  The rounding itself is
// integers (sr_code): the hardware's stochastic conversions are not used
// (DESIGN.md §11.15 says why).
//
// Rotation: the butterflies of h = 1, 2 run inside a lane's four words; h = 4,
// 8, 16 are exchanges with lanes l ^ 1, l ^ 2 (DPP quad_perm) and l ^ 4
// (ds_swizzle, bit mode: the crossbar, no LDS memory).  The lane whose bit is
// clear keeps a + b and its partner a - b: each is (own, sign flipped in the
// upper lane) + other, one IEEE add.  A group's four sign words, one a j, are
// one Philox call a lane — lane l computes block j = l % 4's — handed round
// the quad by DPP broadcasts.  A last block of fewer than 32 elements is not
// rotated; its lanes still take part in every exchange.
#include "bpsr_cast_sr.h"
#include "bpsr_mx_lanes.h"

namespace bpsr {

namespace {

// and_mask 0x1f, or_mask 0, xor_mask 4
constexpr int kSwizzleXor4 = (4 << 10) | 0x1f;

struct Xor1 {
  __device__ __forceinline__ static uint32_t get(uint32_t x) { return dpp<kDppXor1>(x); }
};
struct Xor2 {
  __device__ __forceinline__ static uint32_t get(uint32_t x) { return dpp<kDppXor2>(x); }
};
struct Xor4 {
  __device__ __forceinline__ static uint32_t get(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, kSwizzleXor4);
  }
};

// One butterfly stage across lanes: `upper` — this lane holds the pair's b.
template <class X>
__device__ __forceinline__ void stage(float (&x)[4], bool upper) {
  const uint32_t flip = upper ? 0x80000000u : 0u;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float other = bitcast<float>(X::get(bitcast<uint32_t>(x[e])));
    x[e] = bitcast<float>(bitcast<uint32_t>(x[e]) ^ flip) + other;
  }
}

// The unnormalised Walsh-Hadamard transform of the block this lane's group
// holds, h = 1, 2, 4, 8, 16 in this order.
__device__ __forceinline__ void hadamard32(float (&x)[4], uint32_t lane) {
  const float a0 = x[0] + x[1], a1 = x[0] - x[1], a2 = x[2] + x[3], a3 = x[2] - x[3];
  x[0] = a0 + a2;
  x[2] = a0 - a2;
  x[1] = a1 + a3;
  x[3] = a1 - a3;
  stage<Xor1>(x, (lane & 1) != 0);
  stage<Xor2>(x, (lane & 2) != 0);
  stage<Xor4>(x, (lane & 4) != 0);
}

// The sign words of the lane's four blocks: block j of the tile's group is
// block first_block + 32 j + lane / 8 of the tensor.
__device__ __forceinline__ void sign_words(uint32_t first_block, uint32_t lane, uint32_t step,
                                           uint32_t rot_key, uint32_t (&w)[4]) {
  const uint32_t own =
      (uint32_t)philox2x32_10(first_block + (lane & 3) * 32 + lane / 8, step, rot_key);
  w[0] = dpp<0x00>(own);
  w[1] = dpp<0x55>(own);
  w[2] = dpp<0xAA>(own);
  w[3] = dpp<0xFF>(own);
}

// 0x80000000 where bit 4 (lane % 8) + e of the block's word is set.
__device__ __forceinline__ uint32_t sign_of(uint32_t w, uint32_t lane, int e) {
  return (w >> (4 * (lane & 7) + (uint32_t)e)) << 31;
}

}  // namespace

template <int BITS, bool ROTATE>
__global__ __launch_bounds__(kBlock) void mx_sr_compress_kernel(MxSrCompress p) {
  __shared__ __attribute__((aligned(16))) unsigned char sx[kMxTileBlocks];
  // grid == nrecs: no bounds test in front of the record load
  const MxRec& r = p.recs[blockIdx.x];
  const unsigned char* const g = r.a;
  const uint32_t seg = r.seg, e0 = r.e0, count = r.count, flags = r.flags;
  unsigned char* const payload = p.segs[seg].payload;
  const uint64_t nelem = p.segs[seg].nelem;
  const uint32_t key = p.segs[seg].key, rot_key = p.segs[seg].rot_key, step = p.step;
  asm volatile("" ::"s"(g), "s"(e0), "s"(count), "s"(flags), "s"(payload), "s"(nelem), "s"(key),
               "s"(rot_key), "s"(step));
  const uint32_t lane = threadIdx.x;
  const bool vec = (flags & kMxVec) != 0, al = (flags & kMxAligned) != 0;
  uint32_t c[4][4];
  if (vec && count == kMxTile) {
    const auto rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(g), 0,
                                                      kTileBytes, 0x00020000);
    vec16 x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      x[j] = bitcast<vec16>(
          __builtin_amdgcn_raw_buffer_load_b128(rg, (int)vector_of(j, lane) * 16, 0, kLdAux));
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) c[j][e] = x[j].w[e];
  } else {
    // a ragged or misaligned tile: an element past count is not read and is +0.0
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t p0 = vector_of(j, lane) * 4;
      if (vec && p0 + 4 <= count) {
        const vec16 x = ld16<true>(g + (uint64_t)p0 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) c[j][e] = x.w[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          c[j][e] = 0;
          if (p0 + e < count) c[j][e] = ld_e<uint32_t>(g + (uint64_t)(p0 + e) * 4, al);
        }
      }
    }
  }
  if (e0 == 0 && lane == 0) {
    vec16 hd;
    hd.w[0] = BITS;
    hd.w[1] = (uint32_t)nelem;
    hd.w[2] = (uint32_t)(nelem >> 32);
    hd.w[3] = ROTATE ? 1u : 0u;
    st16<false>(payload, hd);
  }
  unsigned char* const scales = payload + kMxHeader + e0 / kMxBlock;
  unsigned char* const codes = payload + mx_codes_at(nelem) + (uint64_t)e0 * BITS / 8;
  // where the tile's codes and scales end, padding included
  const uint32_t code_end = (uint32_t)mx_align16(mx_code_bytes(count, BITS));
  const uint32_t scale_end = (uint32_t)mx_align16(mx_scale_bytes(count));
  uint32_t sw[4] = {0, 0, 0, 0};
  if constexpr (ROTATE) sign_words(e0 / kMxBlock, lane, step, rot_key, sw);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t p0 = vector_of(j, lane) * 4;
    if constexpr (ROTATE) {
      float x[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] = bitcast<float>(c[j][e] ^ sign_of(sw[j], lane, e));
      hadamard32(x, lane);
      // the block's 32 elements all lie inside the segment
      const bool whole = (p0 & ~(kMxBlock - 1)) + kMxBlock <= count;
#pragma unroll
      for (int e = 0; e < 4; ++e) c[j][e] = whole ? bitcast<uint32_t>(x[e]) : c[j][e];
    }
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t k = c[j][e] & kKeyMask;
      m = k > m ? k : m;
    }
    const uint32_t K = block_max(m), E = K >> 23;
    const bool bad = E == 255;  // an inf or a NaN in the block
    // one more where 2^emax times the largest mantissa would pass the format's max
    const uint32_t Eb = E + ((K & 0x7fffffu) > SrFmt<BITS>::kMant ? 1u : 0u);
    const uint32_t X = bad ? 255u : (Eb > SrFmt<BITS>::kEmax ? Eb - SrFmt<BITS>::kEmax : 0u);
    const float inv = bitcast<float>((254u - (bad ? 127u : X)) << 23);
    const uint64_t bits = philox2x32_10((e0 >> 2) + vector_of(j, lane), step, key);
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t v = bitcast<uint32_t>(bitcast<float>(c[j][e]) * inv);
      const uint32_t q = sr_code<BITS>(v, (uint32_t)(bits >> (16 * e)) & 0xffffu);
      w |= (bad ? 0u : q) << (e * BITS);
    }
    if constexpr (BITS == 8) {
      if (p0 < code_end) *reinterpret_cast<uint32_t*>(codes + p0) = w;
    } else {
      // the odd neighbour's 16 bits beside this lane's: a dword an even lane
      const uint32_t both = w | dpp<kDppXor1>(w) << 16;
      if (!(lane & 1) && p0 / 2 < code_end) *reinterpret_cast<uint32_t*>(codes + p0 / 2) = both;
    }
    if ((lane & 7) == 0) sx[p0 / kMxBlock] = (unsigned char)X;
  }
  __syncthreads();
  if (lane * 16 < scale_end)
    st16<false>(scales + lane * 16, bitcast<vec16>(*reinterpret_cast<const u4*>(&sx[lane * 16])));
}

// bpsr_k_mx.hip's fold — sources kGroup at a time, every load of a group issued
// ahead of its first add — then the rotation undone in registers.
template <int BITS, int POL>
__global__ __launch_bounds__(kBlock) void mx_rht_fold_kernel(MxRhtFold p) {
  constexpr int kGroup = 8;
  const MxRec& r = p.recs[blockIdx.x];
  unsigned char* const out = r.a;
  const uint32_t seg = r.seg, e0 = r.e0, count = r.count, flags = r.flags;
  // sizes come from the plan, never from a header
  const uint64_t nelem = p.segs[seg].nelem;
  const uint32_t rot_key = p.segs[seg].rot_key, step = p.step;
  const int nsrc = p.nsrc;
  asm volatile("" ::"s"(out), "s"(seg), "s"(e0), "s"(count), "s"(flags), "s"(nelem), "s"(nsrc),
               "s"(rot_key), "s"(step));
  const unsigned char* const* const row = p.srcs + (uint64_t)seg * (uint32_t)nsrc;
  const uint64_t scales_at = kMxHeader + e0 / kMxBlock;
  const uint64_t codes_at = mx_codes_at(nelem) + (uint64_t)e0 * BITS / 8;
  const uint32_t lane = threadIdx.x;
  float acc[4][4];
  bool bad[4] = {false, false, false, false};
  for (int s0 = 0; s0 < nsrc; s0 += kGroup) {
    uint32_t w[kGroup][4], X[kGroup][4];
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
      if (s0 + k >= nsrc) break;
      const unsigned char* const src = row[s0 + k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t p0 = vector_of(j, lane) * 4;
        w[k][j] = 0;
        X[k][j] = 0;
        // p0 < count: the lane's codes and its block's scale lie inside the payload
        if (p0 < count) {
          if constexpr (BITS == 8) {
            w[k][j] = __builtin_nontemporal_load(
                reinterpret_cast<const uint32_t*>(src + codes_at + p0));
          } else {
            w[k][j] = __builtin_nontemporal_load(
                reinterpret_cast<const uint16_t*>(src + codes_at + p0 / 2));
          }
          X[k][j] = __builtin_nontemporal_load(src + scales_at + p0 / kMxBlock);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
      if (s0 + k >= nsrc) break;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bad[j] = bad[j] || X[k][j] == 255;
        const float sc = scale_of(X[k][j]);
        float f[4];
        decode4<BITS>(w[k][j], f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = f[e] * sc;
          acc[j][e] = s0 + k == 0 ? d : acc[j][e] + d;
        }
      }
    }
  }
  const bool div = p.divisor > 1;
  const float fd = (float)p.divisor;
  const bool vec = (flags & kMxVec) != 0, al = (flags & kMxAligned) != 0;
  const bool full = vec && count == kMxTile;
  uint32_t sw[4];
  sign_words(e0 / kMxBlock, lane, step, rot_key, sw);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t p0 = vector_of(j, lane) * 4;
    float z[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) z[e] = acc[j][e];
    hadamard32(z, lane);
    const bool whole = (p0 & ~(kMxBlock - 1)) + kMxBlock <= count;
    vec16 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float back =
          bitcast<float>(bitcast<uint32_t>(z[e] * 0.03125f) ^ sign_of(sw[j], lane, e));
      const float t = whole ? back : acc[j][e];
      // a source's X == 255 anywhere in the block: the NaN in these bits
      o.w[e] = bad[j] ? kNaN : bitcast<uint32_t>(div ? t / fd : t);
    }
    if (full) {
      const auto ro = __builtin_amdgcn_make_buffer_rsrc(out, 0, kTileBytes, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(o), ro, (int)p0 * 4, 0, kStAux<POL>);
    } else if (vec && p0 + 4 <= count) {
      st16<true>(out + (uint64_t)p0 * 4, o);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e < count) st_e<uint32_t>(out + (uint64_t)(p0 + e) * 4, o.w[e], al);
    }
  }
}

hipError_t launch_mx_sr_compress(const MxSrCompress& p, uint32_t bits, bool rotate,
                                 hipStream_t s) {
  if (p.nrecs == 0) return hipSuccess;
  auto go = [&](auto B, auto R) -> hipError_t {
    hipLaunchKernelGGL((mx_sr_compress_kernel<decltype(B)::value, decltype(R)::value>),
                       dim3(p.nrecs), dim3(kBlock), 0, s, p);
    return hipGetLastError();
  };
  auto with_rot = [&](auto b) {
    return rotate ? go(b, std::true_type{}) : go(b, std::false_type{});
  };
  return bits == 8 ? with_rot(std::integral_constant<int, 8>{})
                   : with_rot(std::integral_constant<int, 4>{});
}

hipError_t launch_mx_rht_fold(const MxRhtFold& p, uint32_t bits, uint64_t out_bytes,
                              const Tuning& tu, hipStream_t s) {
  if (p.nrecs == 0) return hipSuccess;
  auto go = [&](auto B, auto POL) -> hipError_t {
    hipLaunchKernelGGL((mx_rht_fold_kernel<decltype(B)::value, decltype(POL)::value>),
                       dim3(p.nrecs), dim3(kBlock), 0, s, p);
    return hipGetLastError();
  };
  auto with_pol = [&](auto b) {
    return cast_store_pol(tu, out_bytes) == kPolWt ? go(b, std::integral_constant<int, kPolWt>{})
                                                   : go(b, std::integral_constant<int, kPolNt>{});
  };
  return bits == 8 ? with_pol(std::integral_constant<int, 8>{})
                   : with_pol(std::integral_constant<int, 4>{});
}

}  // namespace bpsr
