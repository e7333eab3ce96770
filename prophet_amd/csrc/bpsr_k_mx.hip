// Block-scaled 8- and 4-bit wires with error feedback: the kernels of
// bpsr_mx.h (the definition is prophet_amd/mx.py — one IEEE
// f32 add, two multiplies and a subtract an element, an integer maximum a
// block, no float reduction).
//
//   COMPRESS  c = g + r; per block of 32 the scale byte X from the largest
//             key; the codes of clamp(c 2^(127 - X)); r' = c - f32(code) 2^(X - 127)
//   FOLD      out = (d_0 + d_1 + ... + d_{N-1}) [/ divisor] in registers
//
// Both are one launch, one workgroup a tile record, and wait on nothing.
//
// The lane map is the cast tiles': a workgroup owns 4,096 contiguous elements,
// lane l's j-th b128 vector is vector j * 256 + l, so word [j][e] of a lane is
// element 4 (256 j + l) + e of the tile.  A block of 32 elements is then the
// j-th vectors of eight adjacent lanes, block 32 j + l / 8 of the tile: its
// largest key is a lane's maximum of four and three DPP exchanges inside a row
// of 16 lanes (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror) —
// integers, no LDS, no float compare.  Lanes that hold nothing (a ragged tile)
// carry +0.0, the definition's padding, and take part in every exchange.
//
// The element conversions are the hardware's: v_cvt_pk_fp8_f32 and
// v_cvt_scalef32_pk_fp4_f32 (scale 1.0) round to nearest even and keep the
// sign of zero; the clamp in front of them means neither saturates nor meets a
// NaN.  v_cvt_f32_fp8 and v_cvt_scalef32_pk_f32_fp4 give f32(code) back.
//
// COMPRESS writes: r' over r as the cast tiles do; a lane's four codes as one
// dword (fp8: a wave's j-th store is 256 contiguous bytes) or, fp4, an even
// lane's and its odd neighbour's eight codes as one dword; the tile's 128 scale
// bytes through LDS as eight b128 stores.  A payload is 16-byte aligned and its
// fields are padded to 16 bytes, and a tile starts on a multiple of 4,096
// elements: the code and scale stores are the same dword and b128 stores in a
// ragged last tile, cut at the padded end, where lanes past the segment's end
// write the padding's zeros.
#include "bpsr_mx_lanes.h"

namespace bpsr {

template <int BITS, int POL>
__global__ __launch_bounds__(kBlock) void mx_compress_kernel(MxCompress p) {
  __shared__ __attribute__((aligned(16))) unsigned char sx[kMxTileBlocks];
  // grid == nrecs: no bounds test in front of the record load
  const MxRec& r = p.recs[blockIdx.x];
  const unsigned char* const g = r.a;
  unsigned char* const q = r.b;
  const uint32_t seg = r.seg, e0 = r.e0, count = r.count, flags = r.flags;
  unsigned char* const payload = p.segs[seg].payload;
  const uint64_t nelem = p.segs[seg].nelem;
  asm volatile("" ::"s"(g), "s"(q), "s"(e0), "s"(count), "s"(flags), "s"(payload), "s"(nelem));
  const uint32_t lane = threadIdx.x;
  const bool vec = (flags & kMxVec) != 0, al = (flags & kMxAligned) != 0;
  const bool full = vec && count == kMxTile;
  auto add = [](uint32_t x, uint32_t y) {
    return bitcast<uint32_t>(bitcast<float>(x) + bitcast<float>(y));
  };
  uint32_t c[4][4];
  if (full) {
    const auto rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(g), 0,
                                                      kTileBytes, 0x00020000);
    const auto rq = __builtin_amdgcn_make_buffer_rsrc(q, 0, kTileBytes, 0x00020000);
    vec16 x[4], y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int off = (int)vector_of(j, lane) * 16;
      x[j] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rg, off, 0, kLdAux));
      y[j] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rq, off, 0, kLdAux));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) c[j][e] = add(x[j].w[e], y[j].w[e]);
  } else {
    // a ragged or misaligned tile: an element past count is not read and is +0.0
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t p0 = vector_of(j, lane) * 4;
      if (vec && p0 + 4 <= count) {
        const vec16 x = ld16<true>(g + (uint64_t)p0 * 4);
        const vec16 y = ld16<true>(q + (uint64_t)p0 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) c[j][e] = add(x.w[e], y.w[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          c[j][e] = 0;
          if (p0 + e >= count) continue;
          const uint64_t at = (uint64_t)(p0 + e) * 4;
          c[j][e] = add(ld_e<uint32_t>(g + at, al), ld_e<uint32_t>(q + at, al));
        }
      }
    }
  }
  if (e0 == 0 && lane == 0) {
    vec16 hd;
    hd.w[0] = BITS;
    hd.w[1] = (uint32_t)nelem;
    hd.w[2] = (uint32_t)(nelem >> 32);
    hd.w[3] = 0;
    st16<false>(payload, hd);
  }
  unsigned char* const scales = payload + kMxHeader + e0 / kMxBlock;
  unsigned char* const codes = payload + mx_codes_at(nelem) + (uint64_t)e0 * BITS / 8;
  // where the tile's codes and scales end, padding included
  const uint32_t code_end = (uint32_t)mx_align16(mx_code_bytes(count, BITS));
  const uint32_t scale_end = (uint32_t)mx_align16(mx_scale_bytes(count));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t p0 = vector_of(j, lane) * 4;
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t key = c[j][e] & kKeyMask;
      m = key > m ? key : m;
    }
    const uint32_t E = block_max(m) >> 23;
    const bool bad = E == 255;  // an inf or a NaN in the block
    const uint32_t X = bad ? 255u : (E > MxFmt<BITS>::kEmax ? E - MxFmt<BITS>::kEmax : 0u);
    const float inv = bitcast<float>((254u - (bad ? 127u : X)) << 23), sc = scale_of(X);
    float v[4], f[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = bitcast<float>(c[j][e]) * inv;
      v[e] = bad ? 0.0f
                 : __builtin_fminf(__builtin_fmaxf(t, -MxFmt<BITS>::kMax), MxFmt<BITS>::kMax);
    }
    const uint32_t w = encode4<BITS>(v);
    decode4<BITS>(w, f);
    vec16 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // a non-finite block: d and r' are the NaN in these bits, not a subtract's
      y.w[e] = bad ? kNaN : bitcast<uint32_t>(bitcast<float>(c[j][e]) - f[e] * sc);
    }
    if (full) {
      const auto rq = __builtin_amdgcn_make_buffer_rsrc(q, 0, kTileBytes, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(y), rq, (int)p0 * 4, 0, kStAux<POL>);
    } else if (vec && p0 + 4 <= count) {
      st16<false>(q + (uint64_t)p0 * 4, y);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e < count) st_e<uint32_t>(q + (uint64_t)(p0 + e) * 4, y.w[e], al);
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

// Sources are taken kGroup at a time: every load of a group is issued ahead of
// its first add.
template <int BITS, int POL>
__global__ __launch_bounds__(kBlock) void mx_fold_kernel(MxFold p) {
  constexpr int kGroup = 8;
  const MxRec& r = p.recs[blockIdx.x];
  unsigned char* const out = r.a;
  const uint32_t seg = r.seg, e0 = r.e0, count = r.count, flags = r.flags;
  // sizes come from the plan, never from a header
  const uint64_t nelem = p.segs[seg].nelem;
  const int nsrc = p.nsrc;
  asm volatile("" ::"s"(out), "s"(seg), "s"(e0), "s"(count), "s"(flags), "s"(nelem), "s"(nsrc));
  const unsigned char* const* const row = p.srcs + (uint64_t)seg * (uint32_t)nsrc;
  const uint64_t scales_at = kMxHeader + e0 / kMxBlock;
  const uint64_t codes_at = mx_codes_at(nelem) + (uint64_t)e0 * BITS / 8;
  const uint32_t lane = threadIdx.x;
  float acc[4][4];
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
        const bool bad = X[k][j] == 255;
        const float sc = scale_of(X[k][j]);
        float f[4];
        decode4<BITS>(w[k][j], f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = bad ? bitcast<float>(kNaN) : f[e] * sc;
          acc[j][e] = s0 + k == 0 ? d : acc[j][e] + d;
        }
      }
    }
  }
  const bool div = p.divisor > 1;
  const float fd = (float)p.divisor;
  const bool vec = (flags & kMxVec) != 0, al = (flags & kMxAligned) != 0;
  const bool full = vec && count == kMxTile;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t p0 = vector_of(j, lane) * 4;
    vec16 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o.w[e] = bitcast<uint32_t>(div ? acc[j][e] / fd : acc[j][e]);
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

// f(BITS, POL) with the format and the store policy as std::integral_constants.
template <class F>
static hipError_t mx_dispatch(uint32_t bits, int pol, F&& f) {
  auto with_pol = [&](auto b) {
    return pol == kPolWt ? f(b, std::integral_constant<int, kPolWt>{})
                         : f(b, std::integral_constant<int, kPolNt>{});
  };
  return bits == 8 ? with_pol(std::integral_constant<int, 8>{})
                   : with_pol(std::integral_constant<int, 4>{});
}

hipError_t launch_mx_compress(const MxCompress& p, uint32_t bits, uint64_t resid_bytes,
                              const Tuning& tu, hipStream_t s) {
  if (p.nrecs == 0) return hipSuccess;
  return mx_dispatch(bits, cast_store_pol(tu, resid_bytes), [&](auto B, auto POL) -> hipError_t {
    hipLaunchKernelGGL((mx_compress_kernel<decltype(B)::value, decltype(POL)::value>),
                       dim3(p.nrecs), dim3(kBlock), 0, s, p);
    return hipGetLastError();
  });
}

hipError_t launch_mx_fold(const MxFold& p, uint32_t bits, uint64_t out_bytes, const Tuning& tu,
                          hipStream_t s) {
  if (p.nrecs == 0) return hipSuccess;
  return mx_dispatch(bits, cast_store_pol(tu, out_bytes), [&](auto B, auto POL) -> hipError_t {
    hipLaunchKernelGGL((mx_fold_kernel<decltype(B)::value, decltype(POL)::value>), dim3(p.nrecs),
                       dim3(kBlock), 0, s, p);
    return hipGetLastError();
  });
}

}  // namespace bpsr
