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
// The tile's shape is bpsr_cast_ef.h's without the residual: the KV = 2 full
// tile with every load issued before the first use, the lane that loaded a
// 16-byte f32 vector rounds its 4 elements, and only the 2-byte values are
// re-dealt (ds_bpermute).  A lane's vector covers elements i0 .. i0 + 3 of the
// tensor, i0 = first + 4 * (the vector's index in the range).  Where `first`
// (the cut's head) is a multiple of 4 that is one Philox group; where it is
// not (a wide base 4-byte but not 16-byte aligned) the vector straddles groups
// q and q + 1, and the lane takes the 64-bit window at bit 16 * (first & 3)
// of the two groups' 128 bits.  `first & 3` is the same for every vector of a
// launch's tensor (of a plan's record), so the second Philox call sits behind
// a wave-uniform branch.
//
// A template on N, instantiated per wire format in bpsr_k_cast_sr.hip (fp16)
// and bpsr_k_cast_sr_bf16.hip (bf16).
#pragma once

#include <cstring>

#include "bpsr_cast_impl.h"

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
// the range's first element in its tensor, as its Philox group and the shift
// within it, and the key and step.  All wave-uniform.
struct SrSeed {
  uint32_t q0;  // first >> 2
  uint32_t sh;  // first & 3
  uint32_t key, step;
};
__device__ __forceinline__ SrSeed sr_seed(uint64_t first, uint32_t key, uint32_t step) {
  return SrSeed{(uint32_t)(first >> 2), (uint32_t)first & 3u, key, step};
}

// Full tile: cast_tile_full's KV = 2 compress; vector `vec` of the tile holds
// elements first + 4 * vec .. + 3 of the tensor.
template <class N, int U, int POL>
__device__ __forceinline__ void cast_sr_tile_full(const unsigned char* src, unsigned char* dst,
                                                  const SrSeed& sd, int lane) {
  constexpr int kAux = 2;                            // loads: nt
  constexpr int kStAux = POL == kPolWt ? 16 : kAux;  // stores: sc1 or nt
  constexpr int KV = 2, DW = 2;
  constexpr int kHBytes = kBlock * U * 16, kWBytes = kHBytes * KV;
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(src), 0, kWBytes,
                                                    0x00020000);
  const auto rd = __builtin_amdgcn_make_buffer_rsrc(dst, 0, kHBytes, 0x00020000);
  const int l = lane & 63, wave0 = lane & ~63;
  vec16 x[U][KV];
#pragma unroll
  for (int j = 0; j < U; ++j)
#pragma unroll
    for (int v = 0; v < KV; ++v)
      x[j][v] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(
          rs, ((j * kBlock + wave0) * KV + v * 64 + l) * 16, 0, kAux));
  const int vi = l / (64 / KV);
#pragma unroll
  for (int j = 0; j < U; ++j) {
    uint32_t c[KV][DW];
#pragma unroll
    for (int v = 0; v < KV; ++v) {
      const uint32_t vec = (uint32_t)((j * kBlock + wave0) * KV + v * 64 + l);
      sr_vec<N>(x[j][v], sr_bits4(sd.q0 + vec, sd.sh, sd.key, sd.step), c[v]);
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

// The partial last tile: units [u0, nunits) of the vector range (both pointers
// already advanced to the range, whose first element is `sd`'s); a unit past
// nunits is neither read nor written.
template <class N, int U>
__device__ __forceinline__ void cast_sr_tile_guarded(const unsigned char* src, unsigned char* dst,
                                                     uint64_t u0, uint64_t nunits,
                                                     const SrSeed& sd, int lane) {
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const uint64_t u = u0 + (uint64_t)j * kBlock + lane;
    if (u >= nunits) continue;
    vec16 x[2], o;
#pragma unroll
    for (int v = 0; v < 2; ++v) x[v] = ld16<true>(src + (u * 2 + v) * 16);
#pragma unroll
    for (int v = 0; v < 2; ++v)
      sr_vec<N>(x[v], sr_bits4(sd.q0 + (uint32_t)(u * 2 + v), sd.sh, sd.key, sd.step),
                &o.w[2 * v]);
    st16<true>(dst + u * 16, o);
  }
}

// Elements [0, head) and [tail_begin, n_elems), one per thread; element e of
// the range is element first + e of its tensor.
template <class N>
__device__ __forceinline__ void cast_sr_elements(const CastArgs& a, uint64_t first, uint32_t key,
                                                 uint32_t step, uint64_t t, uint64_t stride) {
  const bool al = a.aligned != 0;
  const uint64_t n_scalar = a.head + (a.n_elems - a.tail_begin);
  for (uint64_t s = t; s < n_scalar; s += stride) {
    const uint64_t e = s < a.head ? s : a.tail_begin + (s - a.head);
    const uint16_t w =
        sr_round<N>(ld_e<uint32_t>(a.src + e * 4, al), sr_bits1(first + e, key, step));
    st_e<uint16_t>(a.dst + e * 2, w, al);
  }
}

// ------------------------------------------------------- single launch ----
// cast_kernel's shape: workgroup 0 takes the partial tile and the element
// work, the full tiles follow in address order.
template <class N, int U, int POL>
__global__ __launch_bounds__(kBlock) void cast_sr_kernel(CastArgs a, uint32_t key, uint32_t step) {
  asm volatile("" ::"s"(a.src), "s"(a.dst), "s"(a.nunits), "s"(a.head), "s"(a.grid), "s"(key),
               "s"(step));
  constexpr uint64_t kTileUnits = (uint64_t)kBlock * U;
  const uint64_t full = a.nunits / kTileUnits;
  const bool partial = full * kTileUnits < a.nunits;
  const uint64_t bid = blockIdx.x;
  const int elem_mode = a.nunits == 0 ? 2 : (bid == 0 ? 1 : 0);
  const uint64_t tile = partial ? (bid == 0 ? full : bid - 1) : bid;
  const unsigned char* vsrc = a.src + a.head * 4;
  unsigned char* vdst = a.dst + a.head * 2;
  if (tile < full)
    cast_sr_tile_full<N, U, POL>(vsrc + tile * kTileUnits * 32, vdst + tile * kTileUnits * 16,
                                 sr_seed(a.head + tile * kTileUnits * 8, key, step), threadIdx.x);
  else if (tile * kTileUnits < a.nunits)
    cast_sr_tile_guarded<N, U>(vsrc, vdst, tile * kTileUnits, a.nunits,
                               sr_seed(a.head, key, step), threadIdx.x);
  if (elem_mode == 2)
    cast_sr_elements<N>(a, 0, key, step, (uint64_t)blockIdx.x * kBlock + threadIdx.x,
                        a.grid * kBlock);
  else if (elem_mode == 1)
    cast_sr_elements<N>(a, 0, key, step, threadIdx.x, kBlock);
}

template <class N, int U, int POL>
static hipError_t launch_sr_inst(const CastArgs& a, uint32_t key, uint32_t step, const Tuning& tu,
                                 hipStream_t s) {
  static KernelAttr attr;
  const hipError_t lds_ok =
      allow_lds(attr, reinterpret_cast<const void*>(&cast_sr_kernel<N, U, POL>));
  if (lds_ok != hipSuccess) return lds_ok;
  const int occ = a.grid >= tu.occ_min_tiles ? tu.copy_occ : 0;
  hipLaunchKernelGGL((cast_sr_kernel<N, U, POL>), dim3((uint32_t)a.grid), dim3(kBlock),
                     occ_lds_bytes(occ), s, a, key, step);
  return hipGetLastError();
}

template <class N, int POL>
static hipError_t launch_sr_u(const CastArgs& a, uint32_t key, uint32_t step, int u,
                              const Tuning& tu, hipStream_t s) {
  switch (u) {
    case 1: return launch_sr_inst<N, 1, POL>(a, key, step, tu, s);
    case 2: return launch_sr_inst<N, 2, POL>(a, key, step, tu, s);
    default: return launch_sr_inst<N, 4, POL>(a, key, step, tu, s);
  }
}

// The single cast's launch rule (launch_cast): the tile size is copy_vpt,
// halved while there would be fewer than kMinTiles tiles; occupancy as there;
// the store policy is cache_pol's on the 2 bytes an element written.
template <class N>
static hipError_t launch_compress_sr_t(void* dst, const void* src, size_t nelem, uint32_t key,
                                       uint32_t step, const Tuning& tu, hipStream_t s) {
  CastArgs a;
  std::memset(&a, 0, sizeof(a));
  a.src = static_cast<const unsigned char*>(src);
  a.dst = static_cast<unsigned char*>(dst);
  a.divisor = 1;
  const CastCut c = cast_cut(dst, src, nelem, 4);
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
  Tuning tn = tu;
  tn.nt = 1;  // streaming: every byte is read once
  return cache_pol(tn, (uint64_t)nelem * 2) == kPolWt ? launch_sr_u<N, kPolWt>(a, key, step, u, tu, s)
                                                      : launch_sr_u<N, kPolNt>(a, key, step, u, tu, s);
}

// --------------------------------------------------------- plan launch ----
// cast_plan_kernel's compress over an SR plan: record b and, from the
// parallel array, the index in its segment of the record's first element and
// the segment's key — both read at wave-uniform addresses with no bounds test
// in front (grid == nrecords) — and the same record prefetch, with a third
// lane touching the parallel entry of the workgroup kPrefetchAhead later.
template <class N, int U, int POL>
__global__ __launch_bounds__(kBlock) void cast_sr_plan_kernel(
    const CastRec* __restrict__ table, const CastSrRec* __restrict__ stab, uint32_t nrecords,
    uint32_t step) {
  const CastRec& r = table[blockIdx.x];
  const unsigned char* const wide = r.wide;
  unsigned char* const half = r.half;
  const uint64_t first = stab[blockIdx.x].first;
  const uint32_t key = stab[blockIdx.x].key;
  const uint32_t kind = r.kind, count = r.count, aligned = r.aligned;
  asm volatile("" ::"s"(wide), "s"(half), "s"(first), "s"(key), "s"(kind), "s"(count),
               "s"(aligned), "s"(step));
  uint32_t pf = 0;
  if (threadIdx.x < 3 && blockIdx.x + kPrefetchAhead < nrecords) {
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(table + blockIdx.x + kPrefetchAhead);
    const uint32_t* sp = reinterpret_cast<const uint32_t*>(stab + blockIdx.x + kPrefetchAhead);
    pf = *(threadIdx.x < 2 ? rec + threadIdx.x * 7 : sp);
  }
  if (kind == kTileFull) {
    cast_sr_tile_full<N, U, POL>(wide, half, sr_seed(first, key, step), threadIdx.x);
  } else if (kind == kTilePartial) {
    cast_sr_tile_guarded<N, U>(wide, half, 0, count, sr_seed(first, key, step), threadIdx.x);
  } else {
    CastArgs a;
    a.src = wide;
    a.dst = half;
    a.n_elems = count;  // the range [0, count) as a tail that begins at 0
    a.head = a.nunits = a.tail_begin = 0;
    a.grid = 1;
    a.divisor = 1;
    a.aligned = (int)aligned;
    cast_sr_elements<N>(a, first, key, step, threadIdx.x, kBlock);
  }
  keep_prefetch(pf);
}

template <class N, int U, int POL>
static hipError_t launch_sr_plan_inst(const CastRec* table, const CastSrRec* stab,
                                      uint32_t nrecords, uint32_t step, const Tuning& tu,
                                      hipStream_t s) {
  static KernelAttr attr;
  const hipError_t lds_ok =
      allow_lds(attr, reinterpret_cast<const void*>(&cast_sr_plan_kernel<N, U, POL>));
  if (lds_ok != hipSuccess) return lds_ok;
  const int occ = nrecords >= tu.occ_min_tiles_batch ? tu.copy_occ : 0;
  hipLaunchKernelGGL((cast_sr_plan_kernel<N, U, POL>), dim3(nrecords), dim3(kBlock),
                     occ_lds_bytes(occ), s, table, stab, nrecords, step);
  return hipGetLastError();
}

template <class N, int POL>
static hipError_t launch_sr_plan_u(const CastRec* table, const CastSrRec* stab, uint32_t nrecords,
                                   uint32_t step, int u, const Tuning& tu, hipStream_t s) {
  switch (u) {
    case 1: return launch_sr_plan_inst<N, 1, POL>(table, stab, nrecords, step, tu, s);
    case 2: return launch_sr_plan_inst<N, 2, POL>(table, stab, nrecords, step, tu, s);
    default: return launch_sr_plan_inst<N, 4, POL>(table, stab, nrecords, step, tu, s);
  }
}

template <class N>
static hipError_t launch_cast_plan_sr_t(const CastRec* table, const CastSrRec* stab,
                                        uint32_t nrecords, uint32_t step, int u,
                                        uint64_t out_bytes, const Tuning& tu, hipStream_t s) {
  if (u != 1 && u != 2 && u != 4) return hipErrorInvalidValue;
  Tuning tn = tu;
  tn.nt = 1;  // streaming: every byte is read once
  return cache_pol(tn, out_bytes) == kPolWt
             ? launch_sr_plan_u<N, kPolWt>(table, stab, nrecords, step, u, tu, s)
             : launch_sr_plan_u<N, kPolNt>(table, stab, nrecords, step, u, tu, s);
}

}  // namespace bpsr
