// What the block-scaled kernels (bpsr_k_mx.hip, bpsr_k_mx_sr.hip) share on the
// device: the tile's lane map, the exchanges inside a block's eight lanes, the
// scale constants and the decode of four codes.  bpsr_mx.h has the layout.
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

}  // namespace

}  // namespace bpsr
