// Error-feedback compress (Compression.fp16_ef / bf16_ef,
// byteps_reduce_compress_ef, EF cast plans): the compress of bpsr_cast_impl.h
// with a per-tensor f32 residual that holds what the 2-byte wire could not
// carry and is added back before the next cast.  Per element, wide dtype
// FLOAT32 only, wire format N (fp16 or bf16):
//
//   c  = g + r                       IEEE f32 add, RNE, subnormals kept
//   w  = N(c)                        compress_elem's arithmetic, unchanged
//   b  = f32(w)                      exact
//   r' = isfinite(b) ? c - b : +0.0  f32 subtract; exact, b is c in fewer bits
//
// w goes to the wire buffer, r' replaces r in place: one pass that reads
// 4 + 4 bytes an element and writes 2 + 4.  With r == 0 the wire bytes are
// those of the plain compress (but for g = -0.0, which the IEEE add turns
// into +0.0: -0 + +0 = +0); a residual never holds a non-finite value
// (overflow of the wire format, +-inf and NaN leave bits 0).  Pinned bit for
// bit to the same four lines in torch's CPU ops.
//
// The add and the subtract are the plain IEEE `+` and `-` with f32 denormals
// on — the build's default for gfx950 (no -fgpu-flush-denormals-to-zero, no
// fast-math; Makefile), as the bf16 divide of bpsr_cast_impl.h already relies
// on — and are never contracted (-ffp-contract=off).
//
// f32 only: the residual is f32, so only for an f32 wide side does it share
// the wide operand's vector layout (KV = 2 vectors a unit, 4 elements a
// vector).  That sharing is what lets ONE lane own an element's g and r: the
// residual's b128 load and store use the wide load's own offset in a third
// buffer descriptor, 1 KiB contiguous per wave instruction, and only the
// 2-byte values are re-dealt as in the plain compress.
//
// This header holds what error feedback adds — one element's and one vector's
// arithmetic and the scheme that hands them to the shared compress path.  The
// tiles are bpsr_cast_impl.h's, the kernels and launches bpsr_cast_single.h's
// and bpsr_cast_plan.h's.  A template on N, instantiated per wire format in
// bpsr_k_cast_ef.hip (fp16) and bpsr_k_cast_ef_bf16.hip (bf16).
#pragma once

#include "bpsr_cast_plan.h"
#include "bpsr_cast_single.h"

namespace bpsr {

// One element: the wire value, and the new residual's bits through `rn`.
template <class N>
__device__ __forceinline__ uint16_t ef_elem(uint32_t g, uint32_t r, uint32_t* rn) {
  const float c = bitcast<float>(g) + bitcast<float>(r);
  const uint16_t w = N::from_f32(bitcast<uint32_t>(c));
  const float b = N::to_float(w);
  // finite: the exponent field is not all ones (a test on the bits, so no
  // floating-point mode can fold it away)
  const bool fin = (bitcast<uint32_t>(b) & 0x7f800000u) != 0x7f800000u;
  *rn = fin ? bitcast<uint32_t>(c - b) : 0u;
  return w;
}

// A 16-byte vector of f32 (4 elements): two wire dwords, and q updated in place.
template <class N>
__device__ __forceinline__ void ef_vec(const vec16& x, vec16* q, uint32_t* c) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t lo = ef_elem<N>(x.w[2 * k], q->w[2 * k], &q->w[2 * k]);
    const uint32_t hi = ef_elem<N>(x.w[2 * k + 1], q->w[2 * k + 1], &q->w[2 * k + 1]);
    c[k] = lo | (hi << 16);
  }
}

// The scheme (bpsr_cast_impl.h): the state is the residual pointer, moved with
// the range; the residual is the side operand; the kernels' extra argument is
// `resid`, a plan's parallel array the residual pointer of each record.
template <class N>
struct CastEf {
  using Narrow = N;
  static constexpr bool kSide = true, kPlanSide = true;
  struct State {
    unsigned char* resid;
    __device__ __forceinline__ State at(uint64_t n) const { return State{resid + n * 4}; }
  };
  struct Single {
    CastArgs a;
    unsigned char* resid;
  };
  struct Plan {
    const CastRec* table;
    unsigned char* const* rtab;  // already advanced like the record's own two
    uint32_t nrecords;
  };
  __device__ __forceinline__ static State state(const Single& p) { return State{p.resid}; }
  __device__ __forceinline__ static State state(const Plan& p, uint32_t b) {
    return State{p.rtab[b]};
  }
  template <class P>
  __device__ __forceinline__ static void pin(const P&, const State& st) {
    asm volatile("" ::"s"(st.resid));
  }
  __device__ __forceinline__ static int divisor(const Plan&) { return 1; }
  __device__ __forceinline__ static unsigned char* const* plan_side(const Plan& p) {
    return p.rtab;
  }
  __device__ __forceinline__ static unsigned char* side(const State& st) { return st.resid; }
  __device__ __forceinline__ static void vec(const State&, const vec16& x, vec16* q, uint32_t,
                                             uint32_t* c) {
    ef_vec<N>(x, q, c);
  }
  // a.aligned covers all three operands (cast_cut_ef)
  __device__ __forceinline__ static uint16_t elem(const State& st, uint32_t g, uint64_t e,
                                                  bool al) {
    uint32_t rn;
    const uint16_t w = ef_elem<N>(g, ld_e<uint32_t>(st.resid + e * 4, al), &rn);
    st_e<uint32_t>(st.resid + e * 4, rn, al);
    return w;
  }
};

// `out_bytes` of either launch: 6 an element, wire and residual; the
// residual's stores follow the wire side's policy.
template <class N>
static hipError_t launch_compress_ef_t(void* dst, void* resid, const void* src, size_t nelem,
                                       const Tuning& tu, hipStream_t s) {
  typename CastEf<N>::Single p;
  int u;
  const hipError_t e =
      cast_rule(cast_cut_ef(dst, src, resid, nelem), dst, src, nelem, 1, tu, &p.a, &u);
  if (e != hipSuccess) return e;
  p.resid = static_cast<unsigned char*>(resid);
  return launch_single<CastEf<N>, Wide<kFloat32>, true>(p, u, (uint64_t)nelem * 6, tu, s);
}

template <class N>
static hipError_t launch_cast_plan_ef_t(const CastRec* table, unsigned char* const* rtab,
                                        uint32_t nrecords, int u, uint64_t out_bytes,
                                        const Tuning& tu, hipStream_t s) {
  const typename CastEf<N>::Plan p{table, rtab, nrecords};
  return launch_plan_s<CastEf<N>, Wide<kFloat32>, true>(p, u, out_bytes, tu, s);
}

}  // namespace bpsr
