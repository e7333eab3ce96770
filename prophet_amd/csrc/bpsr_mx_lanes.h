// What the block-scaled kernels (bpsr_k_mx.hip, bpsr_k_mx_sr.hip and, for 2-byte
// tensors, bpsr_k_mx_half.hip) share on the device: the tile's lane map, the
// exchanges inside a block's lanes, the scale constants and the conversions of
// four codes.  bpsr_mx.h has the layout.
#pragma once

#include "bpsr_cast_plan.h"
#include "bpsr_mx.h"

namespace bpsr {

namespace {

constexpr int kLdAux = 2;  // streaming loads: nt
template <int POL>
constexpr int kStAux = POL == kPolWt ? 16 : 2;  // stores: sc1 (write-through) or nt
constexpr uint32_t kTileBytes = kMxTile * 4;
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kKeyMask = 0x7fffffffu;
constexpr uint32_t kNaN = 0x7fc00000u;
// DPP controls: the lane's partners inside a block's eight lanes
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141;

template <int BITS>
struct MxFmt;
template <>
struct MxFmt<8> {
  static constexpr uint32_t kEmax = 8;
  static constexpr float kMax = 448.0f;
};
template <>
struct MxFmt<4> {
  static constexpr uint32_t kEmax = 2;
  static constexpr float kMax = 6.0f;
};

// The stateless wires' view of a format (prophet_amd/mx_sr.py).
template <int BITS>
struct SrFmt;
template <>
struct SrFmt<8> {
  static constexpr uint32_t kEmax = 8, kMant = 0x600000u, kMbits = 3, kBias = 7;
};
template <>
struct SrFmt<4> {
  static constexpr uint32_t kEmax = 2, kMant = 0x400000u, kMbits = 1, kBias = 1;
};

// A lane's j-th vector (f32 tiles) or unit (2-byte tiles) of the tile.
__device__ __forceinline__ uint32_t vector_of(int j, uint32_t lane) {
  return (uint32_t)j * kBlock + lane;
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
}

// The maximum over the block's eight lanes, in every one of them.
__device__ __forceinline__ uint32_t block_max(uint32_t m) {
  uint32_t o = dpp<kDppXor1>(m);
  m = o > m ? o : m;
  o = dpp<kDppXor2>(m);
  m = o > m ? o : m;
  o = dpp<kDppHalfMirror>(m);
  return o > m ? o : m;
}

// 2^(X - 127) from its bits; X == 0 is the subnormal 2^-127.
__device__ __forceinline__ float scale_of(uint32_t X) {
  return bitcast<float>(X ? X << 23 : 0x00400000u);
}

// f32(code) of four codes: fp8 a dword, element e in byte e; fp4 the low 16
// bits, element e in nibble e.
template <int BITS>
__device__ __forceinline__ void decode4(uint32_t w, float (&f)[4]) {
  if constexpr (BITS == 8) {
    f[0] = __builtin_amdgcn_cvt_f32_fp8((int)w, 0);
    f[1] = __builtin_amdgcn_cvt_f32_fp8((int)w, 1);
    f[2] = __builtin_amdgcn_cvt_f32_fp8((int)w, 2);
    f[3] = __builtin_amdgcn_cvt_f32_fp8((int)w, 3);
  } else {
    const f2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 0);
    const f2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 1);
    f[0] = lo.x;
    f[1] = lo.y;
    f[2] = hi.x;
    f[3] = hi.y;
  }
}

// Four values, |v| <= max, to their codes: fp8 a dword, element e in byte e;
// fp4 the low 16 bits, element e in nibble e.
template <int BITS>
__device__ __forceinline__ uint32_t encode4(const float (&v)[4]) {
  if constexpr (BITS == 8) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], w, true);
  } else {
    uint32_t w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, v[0], v[1], 1.0f, 0);
    return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[2], v[3], 1.0f, 1) & 0xffffu;
  }
}

// The code of the f32 bits u, |u| <= max, under 16 random bits: with t the
// magnitude in units of 2^-16 of the local step, offset so that its high part
// is the code, (t + r16) >> 16.
template <int BITS>
__device__ __forceinline__ uint32_t sr_code(uint32_t u, uint32_t r16) {
  constexpr uint32_t mb = SrFmt<BITS>::kMbits, bias = SrFmt<BITS>::kBias, drop = 23 - mb;
  const uint32_t a = u & kKeyMask, e = a >> 23;
  const uint32_t normal = (a >> (drop - 16)) - (((127 - bias) << mb) << 16);
  // below the format's smallest normal: the significand shifted down
  const uint32_t m = (a & 0x7fffffu) | (e ? 0x800000u : 0u);
  uint32_t sh = (151 - bias - mb) - (e > 1u ? e : 1u);
  sh = sh > 40u ? 40u : sh;
  const uint32_t sub = (uint32_t)(((uint64_t)m << 16) >> sh);
  const uint32_t t = e >= 128 - bias ? normal : sub;
  return ((t + r16) >> 16) | ((u >> 31) << (BITS - 1));
}

}  // namespace

}  // namespace bpsr
