// Per-tile device code of the 2-byte casts, shared by the single cast
// (bpsr_cast_single.h; bpsr_k_cast.hip for the fp16 wire, bpsr_k_cast_bf16.hip
// for the bf16 wire) and the cast plan (bpsr_cast_plan.h; bpsr_k_cast_plan.hip,
// bpsr_k_cast_plan_bf16.hip): the wide-side element types, the narrow (wire)
// side's two formats, one element's arithmetic, the compress's rounding scheme
// (plain here; error feedback in bpsr_cast_ef.h, stochastic rounding in
// bpsr_cast_sr.h), the full tile, the guarded partial tile and the element
// loop, each written once over the scheme; and, host side, the store policy,
// the tile-size / policy dispatch and the launch wrapper of every cast kernel.
// What the arithmetic is and why the full tile re-deals its lanes:
// bpsr_k_cast.hip, bpsr_k_cast_bf16.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bpsr_kernels_impl.h"

namespace bpsr {

// Wide-side element: its 16-B vectors per unit, and the exact steps to and
// from f32 bits.  get/put address element e (0..7) of a unit's vectors.
// to_f64: the element's value, exactly (the decompress statistics).
// scale: the element times an f32 multiplier, rounded once to the element's
// type (the scaled decompress): the f32 product for f32 and,
// before from_f32's own rounding, for the 2-byte types; the f64 product for f64.
template <int DT>
struct Wide;

template <>
struct Wide<kFloat32> {
  using E = uint32_t;
  static constexpr int kVecs = 2;
  __device__ static uint32_t to_f32(E x) { return x; }
  __device__ static double to_f64(E x) { return (double)bitcast<float>(x); }
  __device__ static E from_f32(float f) { return bitcast<uint32_t>(f); }
  __device__ static E scale(E v, float m) { return from_f32(bitcast<float>(v) * m); }
  __device__ static E get(const vec16* x, int e) { return x[e >> 2].w[e & 3]; }
  __device__ static void put(vec16* x, int e, E v) { x[e >> 2].w[e & 3] = v; }
};

template <>
struct Wide<kFloat64> {
  using E = uint64_t;
  static constexpr int kVecs = 4;
  // round to f32 first (RNE), as the host conversion does
  __device__ static uint32_t to_f32(E x) { return bitcast<uint32_t>((float)bitcast<double>(x)); }
  __device__ static double to_f64(E x) { return bitcast<double>(x); }
  __device__ static E from_f32(float f) { return bitcast<uint64_t>((double)f); }
  // exact: v has at most 11 significant bits here, m has 24
  __device__ static E scale(E v, float m) {
    return bitcast<uint64_t>(bitcast<double>(v) * (double)m);
  }
  __device__ static E get(const vec16* x, int e) {
    return ((uint64_t)x[e >> 1].w[(e & 1) * 2 + 1] << 32) | x[e >> 1].w[(e & 1) * 2];
  }
  __device__ static void put(vec16* x, int e, E v) {
    x[e >> 1].w[(e & 1) * 2] = (uint32_t)v;
    x[e >> 1].w[(e & 1) * 2 + 1] = (uint32_t)(v >> 32);
  }
};

template <>
struct Wide<kBFloat16> {
  using E = uint16_t;
  static constexpr int kVecs = 1;
  __device__ static uint32_t to_f32(E x) { return (uint32_t)x << 16; }  // exact
  __device__ static double to_f64(E x) { return (double)bitcast<float>(to_f32(x)); }
  __device__ static E from_f32(float f) { return (E)f32_to_bf16_rne(bitcast<uint32_t>(f)); }
  __device__ static E scale(E v, float m) { return from_f32(bitcast<float>(to_f32(v)) * m); }
  __device__ static E get(const vec16* x, int e) {
    return (E)(x[0].w[e >> 1] >> ((e & 1) * 16));
  }
  __device__ static void put(vec16* x, int e, E v) {
    if (e & 1) x[0].w[e >> 1] |= (uint32_t)v << 16;
    else x[0].w[e >> 1] = v;
  }
};

// Wide fp16 under the bf16 wire: widened exactly, narrowed as the fp16 wire's
// compress narrows (RNE, overflow to inf, fp16 subnormals produced).
template <>
struct Wide<kFloat16> {
  using E = uint16_t;
  static constexpr int kVecs = 1;
  __device__ static uint32_t to_f32(E x) { return bitcast<uint32_t>((float)bitcast<_Float16>(x)); }
  __device__ static double to_f64(E x) { return (double)(float)bitcast<_Float16>(x); }
  __device__ static E from_f32(float f) { return (E)f2h_bits(bitcast<uint32_t>(f)); }
  __device__ static E scale(E v, float m) { return from_f32(bitcast<float>(to_f32(v)) * m); }
  __device__ static E get(const vec16* x, int e) {
    return (E)(x[0].w[e >> 1] >> ((e & 1) * 16));
  }
  // ORs into the upper half: elements are put in order, the even one first
  __device__ static void put(vec16* x, int e, E v) {
    if (e & 1) x[0].w[e >> 1] |= (uint32_t)v << 16;
    else x[0].w[e >> 1] = v;
  }
};

// Narrow (wire) side: f32 bits to the 2-byte format, round to nearest even,
// and the exact way back.
struct NarrowF16 {
  __device__ static uint16_t from_f32(uint32_t x) { return (uint16_t)f2h_bits(x); }
  __device__ static float to_float(uint16_t h) { return (float)bitcast<_Float16>(h); }
};

// bf16: the integer RNE of the folds (f32_to_bf16_rne) — it rounds the bits,
// so f32 subnormals are kept whatever the wave's denormal mode — and a shift.
struct NarrowBF16 {
  __device__ static uint16_t from_f32(uint32_t x) { return (uint16_t)f32_to_bf16_rne(x); }
  __device__ static float to_float(uint16_t b) { return bitcast<float>((uint32_t)b << 16); }
};

struct CastArgs {
  const unsigned char* src;
  unsigned char* dst;
  uint64_t n_elems;
  uint64_t head;        // elements before the vector range
  uint64_t nunits;      // 8-element units in the vector range
  uint64_t tail_begin;  // head + 8 * nunits
  uint64_t grid;        // launched workgroups
  int divisor;          // decompress: >= 1
  int aligned;          // both operands element-aligned
};

template <class W, class N>
__device__ __forceinline__ uint16_t compress_elem(typename W::E x) {
  return N::from_f32(W::to_f32(x));
}

// div: the quotient is rounded to the narrow format BEFORE it is widened.  A
// bf16 quotient can be an f32 subnormal (fp16's never is): the divide is the
// plain IEEE `/` with f32 denormals on, the build's default.
template <class W, class N>
__device__ __forceinline__ typename W::E decompress_elem(uint16_t h, bool div, float fd) {
  if (div) h = N::from_f32(bitcast<uint32_t>(N::to_float(h) / fd));
  return W::from_f32(N::to_float(h));
}

// Decompress statistics (byteps_reduce_cast_plan_decompress_stats): what a
// lane has seen of the elements it WRITES, each exactly once — the sum of the
// squares of the finite ones in f64 (a square of a value of at most 24
// significant bits is exact; v_fma_f64 adds it with one rounding) and the
// count of the others.  A compile-time choice: the tiles below take the
// accumulator's type, and under StatNone — every compress, every plain
// decompress — add() is nothing and the code is what it was without it.
// Two more compile-time answers of an accumulator: kStore —
// whether the decompress stores what it computed (StatMeasure: no, the
// statistics of a decompress that writes nothing, each element still
// classified by the lane that would have stored it) — and kScale — whether
// the element is multiplied (W::scale) by the accumulator's `m` on its way out
// (StatScale, the scaled decompress).
struct StatNone {
  static constexpr bool kStore = true, kScale = false;
  template <class W>
  __device__ __forceinline__ void add(typename W::E) {}
};
struct StatAcc {
  static constexpr bool kStore = true, kScale = false;
  double sumsq = 0.0;
  uint32_t nonfinite = 0;
  template <class W>
  __device__ __forceinline__ void add(typename W::E v) {
    const double x = W::to_f64(v);
    const bool fin = __builtin_isfinite(x);
    sumsq = fin ? __builtin_fma(x, x, sumsq) : sumsq;
    nonfinite += fin ? 0u : 1u;
  }
};
struct StatMeasure : StatAcc {
  static constexpr bool kStore = false;
};
struct StatScale {
  static constexpr bool kStore = true, kScale = true;
  float m;
  template <class W>
  __device__ __forceinline__ void add(typename W::E) {}
};
// the accumulator's type behind the tiles' forwarding reference
template <class A>
using AccOf = std::remove_cv_t<std::remove_reference_t<A>>;

// decompress_elem, the element shown to the accumulator on its way out
template <class W, class N, class A>
__device__ __forceinline__ typename W::E decompress_elem(uint16_t h, bool div, float fd, A& acc) {
  typename W::E v = decompress_elem<W, N>(h, div, fd);
  if constexpr (A::kScale) v = W::scale(v, acc.m);
  acc.template add<W>(v);
  return v;
}

template <class W, class N, class A>
__device__ __forceinline__ void decompress_unit(const vec16& h, bool div, float fd, vec16* o,
                                                A& acc) {
#pragma unroll
  for (int e = 0; e < 8; ++e)
    W::put(o, e, decompress_elem<W, N>((uint16_t)(h.w[e >> 1] >> ((e & 1) * 16)), div, fd, acc));
}

template <class W, class N>
__device__ __forceinline__ vec16 compress_unit(const vec16* x) {
  vec16 o;
#pragma unroll
  for (int e = 0; e < 8; e += 2)
    o.w[e >> 1] = (uint32_t)compress_elem<W, N>(W::get(x, e)) |
                  ((uint32_t)compress_elem<W, N>(W::get(x, e + 1)) << 16);
  return o;
}

// Rounding scheme S of the f32 compress: what a lane does with the f32
// elements it loaded.  The tiles, the element loop, the two kernels and the
// launches are written once over it.  A scheme supplies
//   Narrow       the wire format
//   State        wave-uniform; at(n) moves it n elements on, to a range's start
//   kSide        a read-write f32 operand, side(st), lies beside the wide one
//                in the wide operand's vector layout and at its offsets
//   vec          one 16-byte vector of f32 to its 4 wire values in c[0..1];
//                vi: the vector's index in the state's range, q: the side
//                operand's vector, updated in place
//   elem         one element, e: its index in the state's range
//   Single, Plan the kernels' arguments; state() reads the State out of them,
//                pin() keeps the scheme's own scalars in SGPRs
//   kPlanSide    a plan has an array parallel to its records, plan_side(),
//                which the record prefetch's third lane touches
// CastPlain: N::from_f32 per element, no side operand and no state.  The other
// wide dtypes and every decompress take no hook (compress_elem,
// decompress_elem) and run under CastPlain.  Error feedback and stochastic
// rounding: bpsr_cast_ef.h, bpsr_cast_sr.h.
template <class N>
struct CastPlain {
  using Narrow = N;
  static constexpr bool kSide = false, kPlanSide = false;
  struct State {
    __device__ __forceinline__ State at(uint64_t) const { return *this; }
  };
  struct Single {
    CastArgs a;
  };
  struct Plan {
    const CastRec* table;
    uint32_t nrecords;
    int divisor;
  };
  __device__ __forceinline__ static State state(const Single&) { return {}; }
  __device__ __forceinline__ static State state(const Plan&, uint32_t) { return {}; }
  __device__ __forceinline__ static void pin(const Single& p, const State&) {
    asm volatile("" ::"s"(p.a.divisor));
  }
  __device__ __forceinline__ static void pin(const Plan& p, const State&) {
    asm volatile("" ::"s"(p.divisor));
  }
  __device__ __forceinline__ static int divisor(const Plan& p) { return p.divisor; }
  __device__ __forceinline__ static void vec(const State&, const vec16& x, vec16*, uint32_t,
                                             uint32_t* c) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
      c[k] = (uint32_t)N::from_f32(x.w[2 * k]) | ((uint32_t)N::from_f32(x.w[2 * k + 1]) << 16);
  }
  __device__ __forceinline__ static uint16_t elem(const State&, uint32_t g, uint64_t, bool) {
    return N::from_f32(g);
  }
};

// Whether the compress of wide side W goes through the scheme's hooks.
template <class W>
constexpr bool kHooked = std::is_same<W, Wide<kFloat32>>::value;

// Full tile: units [0, kBlock * U) of the tile whose first bytes are h0 (narrow
// side) and w0 (wide side), `st` at its first element; lane handles units
// lane + j * kBlock.  One buffer descriptor per operand sized to the tile,
// 32-bit lane offsets.  `acc` (here and in the two below): the decompress
// statistics of the elements this lane writes — in the re-dealt decompress
// that is the lane that stores the output vector.
template <class S, class W, bool COMPRESS, int U, int POL, class A = StatNone>
__device__ __forceinline__ void cast_tile_full(const unsigned char* src, unsigned char* dst,
                                               const typename S::State& st, bool div, float fd,
                                               int lane, A&& acc = A{}) {
  using N = typename S::Narrow;
  constexpr int kAux = 2;                            // loads: nt
  constexpr int kStAux = POL == kPolWt ? 16 : kAux;  // stores: sc1 (write-through) or nt
  constexpr int KV = W::kVecs;
  constexpr int kHBytes = kBlock * U * 16, kWBytes = kHBytes * KV;
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(src), 0,
                                                    COMPRESS ? kWBytes : kHBytes, 0x00020000);
  const auto rd = __builtin_amdgcn_make_buffer_rsrc(dst, 0, COMPRESS ? kHBytes : kWBytes,
                                                    0x00020000);
  if constexpr (COMPRESS && KV > 1) {
    // The mirror image of the decompress below: load instruction v reads the
    // wave's input vectors v * 64 + l (1 KiB contiguous), each lane rounds the
    // elements it loaded into c[v] — through the scheme's hook for f32 — and
    // stores a side vector back at the offset it was loaded from, and lane l
    // collects the 2-byte values of ITS unit (vectors l * KV + s, all in load
    // l / (64 / KV)) from the lanes that hold them.  Every load of the tile,
    // the side operand's included, is issued before the first use; every
    // element is rounded exactly once, by the lane that loaded it.
    constexpr bool kSide = kHooked<W> && S::kSide;
    constexpr int DW = 4 / KV;
    const int l = lane & 63, wave0 = lane & ~63;
    unsigned char* side = nullptr;
    if constexpr (kSide) side = S::side(st);
    const auto rr = __builtin_amdgcn_make_buffer_rsrc(side, 0, kWBytes, 0x00020000);
    vec16 x[U][KV], q[U][KV];
#pragma unroll
    for (int j = 0; j < U; ++j)
#pragma unroll
      for (int v = 0; v < KV; ++v) {
        const int off = ((j * kBlock + wave0) * KV + v * 64 + l) * 16;
        x[j][v] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, kAux));
        if constexpr (kSide)
          q[j][v] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rr, off, 0, kAux));
      }
    const int vl = l / (64 / KV);
#pragma unroll
    for (int j = 0; j < U; ++j) {
      uint32_t c[KV][DW];
#pragma unroll
      for (int v = 0; v < KV; ++v) {
        const int vi = (j * kBlock + wave0) * KV + v * 64 + l;
        if constexpr (kHooked<W>) {
          S::vec(st, x[j][v], &q[j][v], (uint32_t)vi, c[v]);
        } else {
#pragma unroll
          for (int k = 0; k < DW; ++k)
            c[v][k] = (uint32_t)compress_elem<W, N>(W::get(&x[j][v], 2 * k)) |
                      ((uint32_t)compress_elem<W, N>(W::get(&x[j][v], 2 * k + 1)) << 16);
        }
        if constexpr (kSide)
          __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(q[j][v]), rr, vi * 16, 0, kStAux);
      }
      vec16 o;
#pragma unroll
      for (int s = 0; s < KV; ++s) {
        const int from = ((l * KV + s) & 63) * 4;
#pragma unroll
        for (int k = 0; k < DW; ++k) {
          uint32_t r = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)c[0][k]);
#pragma unroll
          for (int v = 1; v < KV; ++v) {
            const uint32_t t = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)c[v][k]);
            r = vl == v ? t : r;
          }
          o.w[s * DW + k] = r;
        }
      }
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(o), rd, (j * kBlock + lane) * 16, 0,
                                             kStAux);
    }
  } else if constexpr (COMPRESS) {
    // a 2-byte wide side: the lane's one vector is its unit, nothing to re-deal
    vec16 x[U][KV];
#pragma unroll
    for (int j = 0; j < U; ++j)
#pragma unroll
      for (int v = 0; v < KV; ++v)
        x[j][v] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(
            rs, ((j * kBlock + lane) * KV + v) * 16, 0, kAux));
#pragma unroll
    for (int j = 0; j < U; ++j)
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(compress_unit<W, N>(x[j])), rd,
                                             (j * kBlock + lane) * 16, 0, kStAux);
  } else {
    vec16 h[U];
#pragma unroll
    for (int j = 0; j < U; ++j)
      h[j] = bitcast<vec16>(
          __builtin_amdgcn_raw_buffer_load_b128(rs, (j * kBlock + lane) * 16, 0, kAux));
    if constexpr (KV > 1) {
      // Lane-private stores would leave each store instruction writing 16 of
      // every 16 * KV bytes — a fraction of each 128-B line per instruction,
      // measured 0.53 (no divide) to 0.59 of the roofline for f32, so it was
      // the store pattern and not the divide that bound it; re-dealt, 0.75
      // with or without the divide.  So the wave's 64 units are
      // re-dealt before the widen: store instruction v writes the wave's
      // output vectors v * 64 + l, 1 KiB contiguous, and lane l fetches the
      // fp16 values of that vector from the lane that loaded them (unit
      // (v * 64 + l) / KV, its sub-vector (v * 64 + l) % KV) by ds_bpermute —
      // the halves travel, 2 bytes an element, and each element is still
      // divided and widened exactly once.  Full tiles only: every lane is
      // active.
      constexpr int EPV = 8 / KV;  // elements per output vector
      const int l = lane & 63, wave0 = lane & ~63;
#pragma unroll
      for (int j = 0; j < U; ++j) {
#pragma unroll
        for (int v = 0; v < KV; ++v) {
          const int g = v * 64 + l;
          const int from = (g / KV) * 4, sub = g % KV;
          uint32_t w[4];
#pragma unroll
          for (int k = 0; k < 4; ++k)
            w[k] = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)h[j].w[k]);
          // the EPV halves of sub-vector `sub`: dwords [sub * EPV / 2, + EPV / 2)
          uint32_t d[EPV / 2];
#pragma unroll
          for (int k = 0; k < EPV / 2; ++k) {
            d[k] = w[k];
#pragma unroll
            for (int s = 1; s < KV; ++s) d[k] = sub == s ? w[s * (EPV / 2) + k] : d[k];
          }
          vec16 o{};
#pragma unroll
          for (int e = 0; e < EPV; ++e)  // e < EPV: all within the one vector
            W::put(&o, e,
                   decompress_elem<W, N>((uint16_t)(d[e >> 1] >> ((e & 1) * 16)), div, fd, acc));
          if constexpr (AccOf<A>::kStore)
            __builtin_amdgcn_raw_buffer_store_b128(
                bitcast<u4>(o), rd, ((j * kBlock + wave0) * KV + g) * 16, 0, kStAux);
        }
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      vec16 o[KV];
      decompress_unit<W, N>(h[j], div, fd, o, acc);
      if constexpr (AccOf<A>::kStore) {
#pragma unroll
        for (int v = 0; v < KV; ++v)
          __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(o[v]), rd,
                                                 ((j * kBlock + lane) * KV + v) * 16, 0, kStAux);
      }
    }
  }
}

// The partial last tile: units [u0, nunits) of the vector range (src / dst
// already advanced to the range, `st` at its first element); a unit past
// nunits is neither read nor written.
template <class S, class W, bool COMPRESS, int U, class A = StatNone>
__device__ __forceinline__ void cast_tile_guarded(const unsigned char* src, unsigned char* dst,
                                                  const typename S::State& st, uint64_t u0,
                                                  uint64_t nunits, bool div, float fd, int lane,
                                                  A&& acc = A{}) {
  using N = typename S::Narrow;
  constexpr int KV = W::kVecs;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const uint64_t u = u0 + (uint64_t)j * kBlock + lane;
    if (u >= nunits) continue;
    if constexpr (COMPRESS && kHooked<W>) {
      vec16 x[KV], q[KV], o;
#pragma unroll
      for (int v = 0; v < KV; ++v) {
        x[v] = ld16<true>(src + (u * KV + v) * 16);
        if constexpr (S::kSide) q[v] = ld16<true>(S::side(st) + (u * KV + v) * 16);
      }
#pragma unroll
      for (int v = 0; v < KV; ++v) {
        S::vec(st, x[v], &q[v], (uint32_t)(u * KV + v), &o.w[2 * v]);
        if constexpr (S::kSide) st16<true>(S::side(st) + (u * KV + v) * 16, q[v]);
      }
      st16<true>(dst + u * 16, o);
    } else if constexpr (COMPRESS) {
      vec16 x[KV];
#pragma unroll
      for (int v = 0; v < KV; ++v) x[v] = ld16<true>(src + (u * KV + v) * 16);
      st16<true>(dst + u * 16, compress_unit<W, N>(x));
    } else {
      vec16 o[KV];
      decompress_unit<W, N>(ld16<true>(src + u * 16), div, fd, o, acc);
      if constexpr (AccOf<A>::kStore) {
#pragma unroll
        for (int v = 0; v < KV; ++v) st16<true>(dst + (u * KV + v) * 16, o[v]);
      }
    }
  }
}

// Elements [0, head) and [tail_begin, n_elems), one per thread; `st` at
// element 0.  a.aligned covers every operand, a side operand included.
template <class S, class W, bool COMPRESS, class A = StatNone>
__device__ __forceinline__ void cast_elements(const CastArgs& a, const typename S::State& st,
                                              bool div, float fd, uint64_t t, uint64_t stride,
                                              A&& acc = A{}) {
  using N = typename S::Narrow;
  using E = typename W::E;
  const bool al = a.aligned != 0;
  const uint64_t n_scalar = a.head + (a.n_elems - a.tail_begin);
  for (uint64_t s = t; s < n_scalar; s += stride) {
    const uint64_t e = s < a.head ? s : a.tail_begin + (s - a.head);
    if constexpr (COMPRESS && kHooked<W>)
      st_e<uint16_t>(a.dst + e * 2, S::elem(st, ld_e<E>(a.src + e * sizeof(E), al), e, al), al);
    else if constexpr (COMPRESS)
      st_e<uint16_t>(a.dst + e * 2, compress_elem<W, N>(ld_e<E>(a.src + e * sizeof(E), al)), al);
    else if constexpr (AccOf<A>::kStore)
      st_e<E>(a.dst + e * sizeof(E),
              decompress_elem<W, N>(ld_e<uint16_t>(a.src + e * 2, al), div, fd, acc), al);
    else
      (void)decompress_elem<W, N>(ld_e<uint16_t>(a.src + e * 2, al), div, fd, acc);
  }
}

// ---------------------------------------------------------- host side ----
// Store policy of a streaming launch (every byte is read once) that writes
// `out_bytes`: write-through below Tuning::wt_max_bytes, nt from there on.
inline int cast_store_pol(const Tuning& tu, uint64_t out_bytes) {
  Tuning tn = tu;
  tn.nt = 1;
  return cache_pol(tn, out_bytes);
}

// f(U, POL) with the tile size u (1, 2 or 4) and the store policy as
// std::integral_constants.
template <class F>
static hipError_t cast_dispatch(int u, int pol, F&& f) {
  auto with_pol = [&](auto p) {
    switch (u) {
      case 1: return f(std::integral_constant<int, 1>{}, p);
      case 2: return f(std::integral_constant<int, 2>{}, p);
      default: return f(std::integral_constant<int, 4>{}, p);
    }
  };
  return pol == kPolWt ? with_pol(std::integral_constant<int, kPolWt>{})
                       : with_pol(std::integral_constant<int, kPolNt>{});
}

// One workgroup per tile or record; residency Tuning::copy_occ from
// `occ_min_tiles` workgroups on.
template <auto KERNEL, class A>
static hipError_t launch_cast_kernel(const A& args, uint64_t grid, uint32_t occ_min_tiles,
                                     const Tuning& tu, hipStream_t s) {
  static KernelAttr attr;
  const hipError_t lds_ok = allow_lds(attr, reinterpret_cast<const void*>(KERNEL));
  if (lds_ok != hipSuccess) return lds_ok;
  const int occ = grid >= occ_min_tiles ? tu.copy_occ : 0;
  hipLaunchKernelGGL(KERNEL, dim3((uint32_t)grid), dim3(kBlock), occ_lds_bytes(occ), s, args);
  return hipGetLastError();
}

}  // namespace bpsr
