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
// 2-byte values are re-dealt (ds_bpermute) as in the plain compress.
//
// A template on N, instantiated per wire format in bpsr_k_cast_ef.hip (fp16)
// and bpsr_k_cast_ef_bf16.hip (bf16).
#pragma once

#include <cstdlib>
#include <cstring>

#include "bpsr_cast_impl.h"

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

// Full tile: cast_tile_full's KV = 2 compress with the residual beside the wide
// operand.  Every load, the residual's included, is issued before the first
// use; the lane that loaded an element computes c, w and r' for it, exactly
// once, and stores the r' vector back at the offset it was loaded from.
// POL: store policy of the wire side, RPOL: of the residual.
template <class N, int U, int POL, int RPOL>
__device__ __forceinline__ void cast_ef_tile_full(const unsigned char* src, unsigned char* resid,
                                                  unsigned char* dst, int lane) {
  constexpr int kAux = 2;                             // loads: nt
  constexpr int kStAux = POL == kPolWt ? 16 : kAux;   // wire stores: sc1 or nt
  constexpr int kRsAux = RPOL == kPolWt ? 16 : kAux;  // residual stores
  constexpr int KV = 2, DW = 2;
  constexpr int kHBytes = kBlock * U * 16, kWBytes = kHBytes * KV;
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(src), 0, kWBytes,
                                                    0x00020000);
  const auto rr = __builtin_amdgcn_make_buffer_rsrc(resid, 0, kWBytes, 0x00020000);
  const auto rd = __builtin_amdgcn_make_buffer_rsrc(dst, 0, kHBytes, 0x00020000);
  const int l = lane & 63, wave0 = lane & ~63;
  vec16 x[U][KV], q[U][KV];
#pragma unroll
  for (int j = 0; j < U; ++j)
#pragma unroll
    for (int v = 0; v < KV; ++v) {
      const int off = ((j * kBlock + wave0) * KV + v * 64 + l) * 16;
      x[j][v] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, kAux));
      q[j][v] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rr, off, 0, kAux));
    }
  const int vi = l / (64 / KV);
#pragma unroll
  for (int j = 0; j < U; ++j) {
    uint32_t c[KV][DW];
#pragma unroll
    for (int v = 0; v < KV; ++v) {
      ef_vec<N>(x[j][v], &q[j][v], c[v]);
      __builtin_amdgcn_raw_buffer_store_b128(
          bitcast<u4>(q[j][v]), rr, ((j * kBlock + wave0) * KV + v * 64 + l) * 16, 0, kRsAux);
    }
    // the re-deal of cast_tile_full: lane l collects the 2-byte values of ITS
    // unit (input vectors l * KV + s) from the lanes that rounded them
    vec16 o;
#pragma unroll
    for (int s = 0; s < KV; ++s) {
      const int from = ((l * KV + s) & 63) * 4;
#pragma unroll
      for (int k = 0; k < DW; ++k) {
        const uint32_t t0 = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)c[0][k]);
        const uint32_t t1 = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)c[1][k]);
        o.w[s * DW + k] = vi == 1 ? t1 : t0;
      }
    }
    __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(o), rd, (j * kBlock + lane) * 16, 0,
                                           kStAux);
  }
}

// The partial last tile: units [u0, nunits) of the vector range (the three
// pointers already advanced to the range); a unit past nunits is neither read
// nor written.
template <class N, int U>
__device__ __forceinline__ void cast_ef_tile_guarded(const unsigned char* src,
                                                     unsigned char* resid, unsigned char* dst,
                                                     uint64_t u0, uint64_t nunits, int lane) {
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const uint64_t u = u0 + (uint64_t)j * kBlock + lane;
    if (u >= nunits) continue;
    vec16 x[2], q[2], o;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      x[v] = ld16<true>(src + (u * 2 + v) * 16);
      q[v] = ld16<true>(resid + (u * 2 + v) * 16);
    }
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      ef_vec<N>(x[v], &q[v], &o.w[2 * v]);
      st16<true>(resid + (u * 2 + v) * 16, q[v]);
    }
    st16<true>(dst + u * 16, o);
  }
}

// Elements [0, head) and [tail_begin, n_elems), one per thread.  a.aligned
// covers all three operands (cast_cut_ef).
__device__ __forceinline__ uint64_t ef_scalar_elem(const CastArgs& a, uint64_t s) {
  return s < a.head ? s : a.tail_begin + (s - a.head);
}

template <class N>
__device__ __forceinline__ void cast_ef_elements(const CastArgs& a, unsigned char* resid,
                                                 uint64_t t, uint64_t stride) {
  const bool al = a.aligned != 0;
  const uint64_t n_scalar = a.head + (a.n_elems - a.tail_begin);
  for (uint64_t s = t; s < n_scalar; s += stride) {
    const uint64_t e = ef_scalar_elem(a, s);
    uint32_t rn;
    const uint16_t w =
        ef_elem<N>(ld_e<uint32_t>(a.src + e * 4, al), ld_e<uint32_t>(resid + e * 4, al), &rn);
    st_e<uint32_t>(resid + e * 4, rn, al);
    st_e<uint16_t>(a.dst + e * 2, w, al);
  }
}

// ------------------------------------------------------- single launch ----
// cast_kernel's shape: workgroup 0 takes the partial tile and the element
// work, the full tiles follow in address order.
template <class N, int U, int POL, int RPOL>
__global__ __launch_bounds__(kBlock) void cast_ef_kernel(CastArgs a, unsigned char* resid) {
  asm volatile("" ::"s"(a.src), "s"(a.dst), "s"(resid), "s"(a.nunits), "s"(a.head), "s"(a.grid));
  constexpr uint64_t kTileUnits = (uint64_t)kBlock * U;
  const uint64_t full = a.nunits / kTileUnits;
  const bool partial = full * kTileUnits < a.nunits;
  const uint64_t bid = blockIdx.x;
  const int elem_mode = a.nunits == 0 ? 2 : (bid == 0 ? 1 : 0);
  const uint64_t tile = partial ? (bid == 0 ? full : bid - 1) : bid;
  const unsigned char* vsrc = a.src + a.head * 4;
  unsigned char* vres = resid + a.head * 4;
  unsigned char* vdst = a.dst + a.head * 2;
  if (tile < full)
    cast_ef_tile_full<N, U, POL, RPOL>(vsrc + tile * kTileUnits * 32,
                                       vres + tile * kTileUnits * 32,
                                       vdst + tile * kTileUnits * 16, threadIdx.x);
  else if (tile * kTileUnits < a.nunits)
    cast_ef_tile_guarded<N, U>(vsrc, vres, vdst, tile * kTileUnits, a.nunits, threadIdx.x);
  if (elem_mode == 2)
    cast_ef_elements<N>(a, resid, (uint64_t)blockIdx.x * kBlock + threadIdx.x, a.grid * kBlock);
  else if (elem_mode == 1)
    cast_ef_elements<N>(a, resid, threadIdx.x, kBlock);
}

template <class N, int U, int POL, int RPOL>
static hipError_t launch_ef_inst(const CastArgs& a, unsigned char* resid, const Tuning& tu,
                                 hipStream_t s) {
  static KernelAttr attr;
  const hipError_t lds_ok =
      allow_lds(attr, reinterpret_cast<const void*>(&cast_ef_kernel<N, U, POL, RPOL>));
  if (lds_ok != hipSuccess) return lds_ok;
  const int occ = a.grid >= tu.occ_min_tiles ? tu.copy_occ : 0;
  hipLaunchKernelGGL((cast_ef_kernel<N, U, POL, RPOL>), dim3((uint32_t)a.grid), dim3(kBlock),
                     occ_lds_bytes(occ), s, a, resid);
  return hipGetLastError();
}

template <class N, int POL, int RPOL>
static hipError_t launch_ef_u(const CastArgs& a, unsigned char* resid, int u, const Tuning& tu,
                              hipStream_t s) {
  switch (u) {
    case 1: return launch_ef_inst<N, 1, POL, RPOL>(a, resid, tu, s);
    case 2: return launch_ef_inst<N, 2, POL, RPOL>(a, resid, tu, s);
    default: return launch_ef_inst<N, 4, POL, RPOL>(a, resid, tu, s);
  }
}

// Store policies of an error-feedback launch that writes `out_bytes` (6 an
// element): the wire side follows cache_pol as the plain casts do.  The
// residual follows it too unless BPSR_EF_RESID_POL names one (1: nt,
// 2: write-through; read once — the measurement's knob).
inline void ef_policies(const Tuning& tu, uint64_t out_bytes, int* pol, int* rpol) {
  static const int forced = [] {
    const char* v = getenv("BPSR_EF_RESID_POL");
    return v ? atoi(v) : 0;
  }();
  Tuning tn = tu;
  tn.nt = 1;  // streaming: every byte is read once
  *pol = cache_pol(tn, out_bytes);
  *rpol = forced == 1 ? kPolNt : forced == 2 ? kPolWt : *pol;
}

// The single cast's launch rule (launch_cast): the tile size is copy_vpt,
// halved while there would be fewer than kMinTiles tiles; occupancy as there.
template <class N>
static hipError_t launch_compress_ef_t(void* dst, void* resid, const void* src, size_t nelem,
                                       const Tuning& tu, hipStream_t s) {
  CastArgs a;
  std::memset(&a, 0, sizeof(a));
  a.src = static_cast<const unsigned char*>(src);
  a.dst = static_cast<unsigned char*>(dst);
  a.divisor = 1;
  const CastCut c = cast_cut_ef(dst, src, resid, nelem);
  a.n_elems = nelem;
  a.aligned = c.aligned;
  a.head = c.head;
  a.nunits = c.nunits;
  a.tail_begin = c.nunits ? c.head + c.nunits * 8 : 0;
  auto tiles = [&a](int u) { return (a.nunits + (uint64_t)kBlock * u - 1) / ((uint64_t)kBlock * u); };
  int u = tu.copy_vpt;
  while (u > 1 && tiles(u) < kMinTiles) u >>= 1;
  uint64_t grid = tiles(u);
  if (grid == 0) {
    grid = (nelem + kBlock - 1) / kBlock;
    if (grid > 65536) grid = 65536;
  }
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  a.grid = grid;
  int pol, rpol;
  ef_policies(tu, (uint64_t)nelem * 6, &pol, &rpol);
  unsigned char* r = static_cast<unsigned char*>(resid);
  if (pol == kPolWt)
    return rpol == kPolWt ? launch_ef_u<N, kPolWt, kPolWt>(a, r, u, tu, s)
                          : launch_ef_u<N, kPolWt, kPolNt>(a, r, u, tu, s);
  return rpol == kPolWt ? launch_ef_u<N, kPolNt, kPolWt>(a, r, u, tu, s)
                        : launch_ef_u<N, kPolNt, kPolNt>(a, r, u, tu, s);
}

// --------------------------------------------------------- plan launch ----
// cast_plan_kernel's compress over an EF plan: record b and, from the
// parallel array, the residual pointer of record b — both read at
// wave-uniform addresses with no bounds test in front (grid == nrecords) —
// and the same record prefetch, with a third lane touching the residual
// pointer of the workgroup kPrefetchAhead later.
template <class N, int U, int POL, int RPOL>
__global__ __launch_bounds__(kBlock) void cast_ef_plan_kernel(
    const CastRec* __restrict__ table, unsigned char* const* __restrict__ rtab,
    uint32_t nrecords) {
  const CastRec& r = table[blockIdx.x];
  const unsigned char* const wide = r.wide;
  unsigned char* const half = r.half;
  unsigned char* const resid = rtab[blockIdx.x];
  const uint32_t kind = r.kind, count = r.count, aligned = r.aligned;
  asm volatile("" ::"s"(wide), "s"(half), "s"(resid), "s"(kind), "s"(count), "s"(aligned));
  uint32_t pf = 0;
  if (threadIdx.x < 3 && blockIdx.x + kPrefetchAhead < nrecords) {
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(table + blockIdx.x + kPrefetchAhead);
    const uint32_t* rp = reinterpret_cast<const uint32_t*>(rtab + blockIdx.x + kPrefetchAhead);
    pf = *(threadIdx.x < 2 ? rec + threadIdx.x * 7 : rp);
  }
  if (kind == kTileFull) {
    cast_ef_tile_full<N, U, POL, RPOL>(wide, resid, half, threadIdx.x);
  } else if (kind == kTilePartial) {
    cast_ef_tile_guarded<N, U>(wide, resid, half, 0, count, threadIdx.x);
  } else {
    CastArgs a;
    a.src = wide;
    a.dst = half;
    a.n_elems = count;  // the range [0, count) as a tail that begins at 0
    a.head = a.nunits = a.tail_begin = 0;
    a.grid = 1;
    a.divisor = 1;
    a.aligned = (int)aligned;
    cast_ef_elements<N>(a, resid, threadIdx.x, kBlock);
  }
  keep_prefetch(pf);
}

template <class N, int U, int POL, int RPOL>
static hipError_t launch_ef_plan_inst(const CastRec* table, unsigned char* const* rtab,
                                      uint32_t nrecords, const Tuning& tu, hipStream_t s) {
  static KernelAttr attr;
  const hipError_t lds_ok =
      allow_lds(attr, reinterpret_cast<const void*>(&cast_ef_plan_kernel<N, U, POL, RPOL>));
  if (lds_ok != hipSuccess) return lds_ok;
  const int occ = nrecords >= tu.occ_min_tiles_batch ? tu.copy_occ : 0;
  hipLaunchKernelGGL((cast_ef_plan_kernel<N, U, POL, RPOL>), dim3(nrecords), dim3(kBlock),
                     occ_lds_bytes(occ), s, table, rtab, nrecords);
  return hipGetLastError();
}

template <class N, int POL, int RPOL>
static hipError_t launch_ef_plan_u(const CastRec* table, unsigned char* const* rtab,
                                   uint32_t nrecords, int u, const Tuning& tu, hipStream_t s) {
  switch (u) {
    case 1: return launch_ef_plan_inst<N, 1, POL, RPOL>(table, rtab, nrecords, tu, s);
    case 2: return launch_ef_plan_inst<N, 2, POL, RPOL>(table, rtab, nrecords, tu, s);
    default: return launch_ef_plan_inst<N, 4, POL, RPOL>(table, rtab, nrecords, tu, s);
  }
}

template <class N>
static hipError_t launch_cast_plan_ef_t(const CastRec* table, unsigned char* const* rtab,
                                        uint32_t nrecords, int u, uint64_t out_bytes,
                                        const Tuning& tu, hipStream_t s) {
  if (u != 1 && u != 2 && u != 4) return hipErrorInvalidValue;
  int pol, rpol;
  ef_policies(tu, out_bytes, &pol, &rpol);
  if (pol == kPolWt)
    return rpol == kPolWt ? launch_ef_plan_u<N, kPolWt, kPolWt>(table, rtab, nrecords, u, tu, s)
                          : launch_ef_plan_u<N, kPolWt, kPolNt>(table, rtab, nrecords, u, tu, s);
  return rpol == kPolWt ? launch_ef_plan_u<N, kPolNt, kPolWt>(table, rtab, nrecords, u, tu, s)
                        : launch_ef_plan_u<N, kPolNt, kPolNt>(table, rtab, nrecords, u, tu, s);
}

}  // namespace bpsr
