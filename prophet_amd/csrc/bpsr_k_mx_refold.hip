// The server round of the block-scaled error-feedback wires (mxfp8_ef,
// mxfp4_ef; the definition is prophet_amd/mx.py's refold):
//
//   REFOLD  c = (d_0 + d_1 + ... + d_{N-1}) + r in registers, then bpsr_k_mx.hip's
//           compress of c: the scale byte X of each block of 32, the codes,
//           r' = c - f32(code) 2^(X - 127) over r, one payload out
//
// One launch a plan, one workgroup a tile record of 4,096 elements; it waits on
// nothing and has no scratch memory: the f32 sum never reaches memory.  The
// lane map, the exchanges and the conversions are bpsr_mx_lanes.h's, so a lane
// decodes, sums, scales and encodes the same sixteen elements — four b128
// vectors of the residual, four code dwords (fp4: halves) and four scale bytes
// a source — and a block's maximum is three DPP exchanges as in the compress.
//
// Order of the memory work in a tile: the residual's four b128 loads go out
// first and stay in flight under the decode; then the sources kGroup at a time,
// every load of a group issued ahead of its first add; the adds run in source
// order (the order is part of the definition).  A source's header is never
// read: sizes come from the plan.
//
// kGroup = 8: a group holds 8 x 8 dwords of codes and scale bytes beside the 16
// accumulators and the 16 residual words (DESIGN.md §11.17 has the compiler's
// register report for gfx950 and what a group of 4 gives instead).
//
// Ragged last tiles and a residual 4 bytes off alignment take the vector and
// element paths of the compress; lanes past `count` carry +0.0 and take part in
// every exchange.  The payload's stores are the compress's: dwords of codes and
// b128 runs of scale bytes through LDS, cut at the padded end of the fields.
#include "bpsr_mx_lanes.h"

namespace bpsr {

namespace {
constexpr int kMxRefoldGroup = 8;
}

template <int BITS, int POL>
__global__ __launch_bounds__(kBlock) void mx_refold_kernel(MxRefold p) {
  constexpr int kGroup = kMxRefoldGroup;
  __shared__ __attribute__((aligned(16))) unsigned char sx[kMxTileBlocks];
  // grid == nrecs: no bounds test in front of the record load
  const MxRec& r = p.recs[blockIdx.x];
  unsigned char* const q = r.a;
  const uint32_t seg = r.seg, e0 = r.e0, count = r.count, flags = r.flags;
  unsigned char* const payload = p.segs[seg].payload;
  // sizes come from the plan, never from a header
  const uint64_t nelem = p.segs[seg].nelem;
  const int nsrc = p.nsrc;
  asm volatile("" ::"s"(q), "s"(seg), "s"(e0), "s"(count), "s"(flags), "s"(payload), "s"(nelem),
               "s"(nsrc));
  // The row of source pointers is read-only for the launch.  Read through the
  // constant address space the pointers arrive by scalar loads: a vector load
  // of a pointer would have to be waited for with vmcnt(0), behind every code
  // and scale load issued before it, and the group's loads would go out one
  // source at a time.
  typedef const unsigned char* SrcPtr;
  const auto* const row = (const __attribute__((address_space(4))) SrcPtr*)(
      p.srcs + (uint64_t)seg * (uint32_t)nsrc);
  const uint64_t scales_at = kMxHeader + e0 / kMxBlock;
  const uint64_t codes_at = mx_codes_at(nelem) + (uint64_t)e0 * BITS / 8;
  const uint32_t lane = threadIdx.x;
  const bool vec = (flags & kMxVec) != 0, al = (flags & kMxAligned) != 0;
  const bool full = vec && count == kMxTile;

  // the residual: issued here, first used after the last source's add
  uint32_t c[4][4];
  if (full) {
    const auto rq = __builtin_amdgcn_make_buffer_rsrc(q, 0, kTileBytes, 0x00020000);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const vec16 y = bitcast<vec16>(
          __builtin_amdgcn_raw_buffer_load_b128(rq, (int)vector_of(j, lane) * 16, 0, kLdAux));
#pragma unroll
      for (int e = 0; e < 4; ++e) c[j][e] = y.w[e];
    }
  } else {
    // a ragged or misaligned tile: an element past count is not read and is +0.0
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t p0 = vector_of(j, lane) * 4;
      if (vec && p0 + 4 <= count) {
        const vec16 y = ld16<true>(q + (uint64_t)p0 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) c[j][e] = y.w[e];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          c[j][e] = p0 + e < count ? ld_e<uint32_t>(q + (uint64_t)(p0 + e) * 4, al) : 0u;
      }
    }
  }

  // The N-way decode and sum, in source order.  Every lane loads: a lane whose
  // vector starts past count reads the tile's first codes and scale instead
  // (count > 0: they lie inside the payload) and drops them, so no load sits
  // under a branch and none writes a register that was cleared ahead of it.
  float acc[4][4] = {};
  for (int s0 = 0; s0 < (count ? nsrc : 0); s0 += kGroup) {
    uint32_t w[kGroup][4], X[kGroup][4];
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
      if (s0 + k >= nsrc) break;
      const unsigned char* const src = row[s0 + k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t p0 = vector_of(j, lane) * 4, at = p0 < count ? p0 : 0u;
        if constexpr (BITS == 8) {
          w[k][j] = __builtin_nontemporal_load(
              reinterpret_cast<const uint32_t*>(src + codes_at + at));
        } else {
          w[k][j] = __builtin_nontemporal_load(
              reinterpret_cast<const uint16_t*>(src + codes_at + at / 2));
        }
        X[k][j] = __builtin_nontemporal_load(src + scales_at + at / kMxBlock);
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
  // c = fold + r: one IEEE add, the compress's first line.  An element past
  // count is the padding's +0.0 whatever a source's pad bits hold.
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t p0 = vector_of(j, lane) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      c[j][e] = p0 + e < count ? bitcast<uint32_t>(acc[j][e] + bitcast<float>(c[j][e])) : 0u;
  }

  if (e0 == 0 && lane == 0) {
    vec16 hd;
    hd.w[0] = BITS;
    hd.w[1] = (uint32_t)nelem;
    hd.w[2] = (uint32_t)(nelem >> 32);
    hd.w[3] = 0;
    st16<false>(payload, hd);
  }
  unsigned char* const scales = payload + scales_at;
  unsigned char* const codes = payload + codes_at;
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
    const bool bad = E == 255;  // a source's X == 255, an overflowed sum, a bad residual
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
      // a non-finite block: r' is the NaN in these bits, not a subtract's
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

hipError_t launch_mx_refold(const MxRefold& p, uint32_t bits, uint64_t resid_bytes,
                            const Tuning& tu, hipStream_t s) {
  if (p.nrecs == 0) return hipSuccess;
  const bool wt = cast_store_pol(tu, resid_bytes) == kPolWt;
  auto go = [&](auto B, auto POL) -> hipError_t {
    hipLaunchKernelGGL((mx_refold_kernel<decltype(B)::value, decltype(POL)::value>),
                       dim3(p.nrecs), dim3(kBlock), 0, s, p);
    return hipGetLastError();
  };
  auto with_pol = [&](auto b) {
    return wt ? go(b, std::integral_constant<int, kPolWt>{})
              : go(b, std::integral_constant<int, kPolNt>{});
  };
  return bits == 8 ? with_pol(std::integral_constant<int, 8>{})
                   : with_pol(std::integral_constant<int, 4>{});
}

}  // namespace bpsr
