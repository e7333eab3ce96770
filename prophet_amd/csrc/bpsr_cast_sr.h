// Stochastic-rounding compress (Compression.fp16_sr / bf16_sr,
// byteps_reduce_compress_sr, SR cast plans): the compress of bpsr_cast_impl.h
// with round-to-nearest-even replaced by rounding up with a probability equal
// to the dropped fraction, so the wire value is right in expectation and no
// state is kept: 4 bytes read and 2 written an element, as the plain compress.
// Wide dtype FLOAT32 only.  The result is a pure function of (bits of g, key,
// step, element index) — no device RNG state — pinned bit for bit to the
// numpy restatement in prophet_amd/sr.py, which is the definition.
//
// Random bits: Philox2x32-10, multiplier 0xD256D193, key increment 0x9E3779B9.
// Element i (0-based in its tensor, whatever its address) takes 16 bits of
// philox(c0 = i >> 2, c1 = step, k = key): X = x0 | x1 << 32 is the group's 64
// bits and r16 = (X >> 16 * (i & 3)) & 0xffff.  The key schedule is
// wave-uniform (scalar); a round is one 32 x 32 -> 64-bit multiply and two
// xors a lane.
//
// bf16 (u = the f32 bits): w = (u + r16) >> 16, never wrapping, unless the
// exponent field is 0xff, where the value is the plain compress's.  fp16: the
// value cut toward zero (lo) plus the carry out of (f + r16), f the dropped
// fraction to 16 bits; sr_round<NarrowF16> below is sr.py's sr_fp16 line by
// line.
//
// The tile is the plain compress's (bpsr_cast_impl.h): the KV = 2 full tile
// with every load issued before the first use, the lane that loaded a 16-byte
// f32 vector rounds its 4 elements, and only the 2-byte values are re-dealt.
// A lane's vector covers elements i0 .. i0 + 3 of the
// tensor, i0 = first + 4 * (the vector's index in the range).  Where `first`
// (the cut's head) is a multiple of 4 that is one Philox group; where it is
// not (a wide base 4-byte but not 16-byte aligned) the vector straddles groups
// q and q + 1, and the lane takes the 64-bit window at bit 16 * (first & 3)
// of the two groups' 128 bits.  `first & 3` is the same for every vector of a
// launch's tensor (of a plan's record), so the second Philox call sits behind
// a wave-uniform branch.
//
// This header holds what stochastic rounding adds — the random bits, one
// element's and one vector's rounding and the scheme that hands them to the
// shared compress path.  The tiles are bpsr_cast_impl.h's, the kernels and
// launches bpsr_cast_single.h's and bpsr_cast_plan.h's.  A template on N,
// instantiated per wire format in bpsr_k_cast_sr.hip (fp16) and
// bpsr_k_cast_sr_bf16.hip (bf16).
#pragma once

#include "bpsr_cast_plan.h"
#include "bpsr_cast_single.h"

namespace bpsr {

constexpr uint32_t kPhiloxM = 0xD256D193u, kPhiloxW = 0x9E3779B9u;

// Philox2x32-10 of counter (c0, c1) under key k, as x0 | x1 << 32.
__device__ __forceinline__ uint64_t philox2x32_10(uint32_t c0, uint32_t c1, uint32_t k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p = (uint64_t)kPhiloxM * c0;
    c0 = (uint32_t)(p >> 32) ^ k ^ c1;
    c1 = (uint32_t)p;
    k += kPhiloxW;
  }
  return (uint64_t)c0 | ((uint64_t)c1 << 32);
}

// The 64 random bits of elements i0 .. i0 + 3: i0 = 4 * q + sh, sh wave-uniform.
__device__ __forceinline__ uint64_t sr_bits4(uint32_t q, uint32_t sh, uint32_t key,
                                             uint32_t step) {
  uint64_t x = philox2x32_10(q, step, key);
  if (sh != 0) {
    const uint64_t y = philox2x32_10(q + 1, step, key);
    x = (x >> (16 * sh)) | (y << (64 - 16 * sh));
  }
  return x;
}

// One element's 16 bits.
__device__ __forceinline__ uint32_t sr_bits1(uint64_t i, uint32_t key, uint32_t step) {
  const uint64_t x = philox2x32_10((uint32_t)(i >> 2), step, key);
  return (uint32_t)(x >> (16 * ((uint32_t)i & 3u))) & 0xffffu;
}

// One element: f32 bits u and 16 random bits to the wire format.
template <class N>
__device__ __forceinline__ uint16_t sr_round(uint32_t u, uint32_t r16);

template <>
__device__ __forceinline__ uint16_t sr_round<NarrowBF16>(uint32_t u, uint32_t r16) {
  if ((u & 0x7f800000u) == 0x7f800000u) return NarrowBF16::from_f32(u);
  return (uint16_t)((u + r16) >> 16);
}

template <>
__device__ __forceinline__ uint16_t sr_round<NarrowF16>(uint32_t u, uint32_t r16) {
  const uint32_t s = (u >> 16) & 0x8000u;
  const uint32_t a = u & 0x7fffffffu;
  const uint32_t e = a >> 23;
  if (e == 0xffu) return NarrowF16::from_f32(u);
  uint32_t lo, f;
  if (e >= 113u) {
    lo = (a >> 13) - 0x1c000u;
    f = (a & 0x1fffu) << 3;
  } else {
    const uint32_t m = (a & 0x7fffffu) | (e ? 0x800000u : 0u);
    const uint32_t sh = 126u - (e > 1u ? e : 1u);
    if (sh >= 40u) {
      lo = 0;
      f = 0;
    } else {
      lo = (uint32_t)((uint64_t)m >> sh);
      f = (uint32_t)((((uint64_t)m << 16) >> sh) & 0xffffu);
    }
  }
  uint32_t h = lo + ((f + r16) >> 16);
  h = h > 0x7c00u ? 0x7c00u : h;
  if (a >= 0x47800000u) h = 0x7c00u;
  return (uint16_t)(s | h);
}

// A 16-byte vector of f32 (4 elements) under the 64 bits `x`: two wire dwords.
template <class N>
__device__ __forceinline__ void sr_vec(const vec16& v, uint64_t x, uint32_t* c) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t w = (uint32_t)(x >> (32 * k));
    const uint32_t lo = sr_round<N>(v.w[2 * k], w & 0xffffu);
    const uint32_t hi = sr_round<N>(v.w[2 * k + 1], w >> 16);
    c[k] = lo | (hi << 16);
  }
}

// What every tile needs beside its two operands: the element index `first` of
// the range's first element in its tensor, the key and the step.  All
// wave-uniform.
struct SrSeed {
  uint64_t first;
  uint32_t key, step;
  __device__ __forceinline__ SrSeed at(uint64_t n) const { return SrSeed{first + n, key, step}; }
};

// The scheme (bpsr_cast_impl.h): the state is the seed; vector vi of a range
// holds elements first + 4 * vi .. + 3 of the tensor, Philox group
// (first >> 2) + vi shifted by first & 3.  The kernels' extra arguments are
// the key and the step; a plan's parallel array gives each record its first
// element's index in its segment and the segment's key.
template <class N>
struct CastSr {
  using Narrow = N;
  static constexpr bool kSide = false, kPlanSide = true;
  using State = SrSeed;
  struct Single {
    CastArgs a;
    uint32_t key, step;
  };
  struct Plan {
    const CastRec* table;
    const CastSrRec* stab;
    uint32_t nrecords;
    uint32_t step;
  };
  __device__ __forceinline__ static State state(const Single& p) { return State{0, p.key, p.step}; }
  __device__ __forceinline__ static State state(const Plan& p, uint32_t b) {
    return State{p.stab[b].first, p.stab[b].key, p.step};
  }
  __device__ __forceinline__ static void pin(const Single& p, const State&) {
    asm volatile("" ::"s"(p.key), "s"(p.step));
  }
  __device__ __forceinline__ static void pin(const Plan& p, const State& st) {
    asm volatile("" ::"s"(st.first), "s"(st.key), "s"(p.step));
  }
  __device__ __forceinline__ static int divisor(const Plan&) { return 1; }
  __device__ __forceinline__ static const CastSrRec* plan_side(const Plan& p) { return p.stab; }
  __device__ __forceinline__ static void vec(const State& sd, const vec16& x, vec16*,
                                             uint32_t vi, uint32_t* c) {
    sr_vec<N>(x, sr_bits4((uint32_t)(sd.first >> 2) + vi, (uint32_t)sd.first & 3u, sd.key, sd.step),
              c);
  }
  __device__ __forceinline__ static uint16_t elem(const State& sd, uint32_t g, uint64_t e, bool) {
    return sr_round<N>(g, sr_bits1(sd.first + e, sd.key, sd.step));
  }
};

// `out_bytes` of either launch: 2 an element.
template <class N>
static hipError_t launch_compress_sr_t(void* dst, const void* src, size_t nelem, uint32_t key,
                                       uint32_t step, const Tuning& tu, hipStream_t s) {
  typename CastSr<N>::Single p;
  int u;
  const hipError_t e = cast_rule(cast_cut(dst, src, nelem, 4), dst, src, nelem, 1, tu, &p.a, &u);
  if (e != hipSuccess) return e;
  p.key = key;
  p.step = step;
  return launch_single<CastSr<N>, Wide<kFloat32>, true>(p, u, (uint64_t)nelem * 2, tu, s);
}

template <class N>
static hipError_t launch_cast_plan_sr_t(const CastRec* table, const CastSrRec* stab,
                                        uint32_t nrecords, uint32_t step, int u,
                                        uint64_t out_bytes, const Tuning& tu, hipStream_t s) {
  const typename CastSr<N>::Plan p{table, stab, nrecords, step};
  return launch_plan_s<CastSr<N>, Wide<kFloat32>, true>(p, u, out_bytes, tu, s);
}

}  // namespace bpsr
