// The SGD step inside the decompress (byteps_reduce_cast_plan_apply_sgd,
// DESIGN.md §11.9): a cast-plan kernel over the CastRec table whose wide
// operand is the f32 PARAMETER and whose side operand, an array of pointers
// parallel to the records exactly as an error-feedback plan's rtab, is the f32
// MOMENTUM buffer.  The gradient — what the decompress would have written — is
// never stored: it lives in registers between the widen and the update.  Per
// element, every line one IEEE f32 operation, RNE, subnormals kept, nothing
// contracted (-ffp-contract=off), wire format N:
//
//   h  = the wire value; divisor > 1: N(f32(h) / divisor)   decompress_elem's
//   g  = f32(h)                                              exact
//   g  = g * mult              with a clip record (the scaled decompress's)
//   g  = g + wd * p            when wd != 0
//   m' = mu * m + g
//   d  = nesterov ? g + mu * m' : m'
//   p' = p - lr * d
//
// p' and m' replace p and m in place: 2 + 4 + 4 bytes read and 4 + 4 written
// an element, 18 B against 6 (the scaled decompress) + 20 (a fused optimizer).
// The three selects (record, wd, nesterov) are wave-uniform run-time values:
// the kernel is instantiated per (wire, U, store policy) alone.
//
// The full tile is the re-dealt f32 decompress of bpsr_cast_impl.h: the lane
// that would store output vector ((j * kBlock + wave0) * KV + g) of the
// gradient holds that vector's 4 values after the ds_bpermute, and the
// parameter's and the momentum's vectors lie at that very offset of their own
// buffer descriptors — one lane owns an element's g, p and m, every load of
// the tile is issued before the first use, and every instruction of a wave
// reads or writes 1 KiB contiguous.
//
// With a clip record and skip_nonfinite, a record whose nonfinite is not 0
// ends every workgroup before any vector load or store: an overflowed step is
// skipped with no host round trip (GradScaler's found_inf).
//
// A template on N, instantiated in bpsr_k_cast_sgd.hip (fp16 wire) and
// bpsr_k_cast_sgd_bf16.hip (bf16 wire).
#pragma once

#include "bpsr_cast_plan.h"

namespace bpsr {

// The step's wave-uniform values.
struct SgdOp {
  float lr, mu, wd, mult;
  bool scale, decay, nesterov;
};

// One element: p and m are replaced by p' and m'.
template <class N>
__device__ __forceinline__ void sgd_elem(uint16_t h, bool div, float fd, const SgdOp& o,
                                         uint32_t& pb, uint32_t& mb) {
  float g = bitcast<float>(decompress_elem<Wide<kFloat32>, N>(h, div, fd));
  const float p = bitcast<float>(pb), m = bitcast<float>(mb);
  if (o.scale) g = g * o.mult;
  if (o.decay) {
    const float t = o.wd * p;
    g = g + t;
  }
  const float t1 = o.mu * m;
  const float mn = t1 + g;
  float d = mn;
  if (o.nesterov) {
    const float t2 = o.mu * mn;
    d = g + t2;
  }
  const float t3 = o.lr * d;
  pb = bitcast<uint32_t>(p - t3);
  mb = bitcast<uint32_t>(mn);
}

// The kernel argument: the plan's table, the momentum pointer of every record
// (already advanced like the record's own two), the hyper-parameters by value
// and the nullable clip record.
struct SgdPlan {
  const CastRec* table;
  unsigned char* const* mtab;
  uint32_t nrecords;
  int divisor;
  float lr, mu, wd;
  int nesterov;
  const byteps_clip_record* rec;
  int skip;
};

// Full tile: kBlock * U units at `half`, their 8 * kBlock * U parameters at
// `par` and momenta at `mom`.  One descriptor per operand sized to the tile.
template <class N, int U, int POL>
__device__ __forceinline__ void sgd_tile_full(const unsigned char* half, unsigned char* par,
                                              unsigned char* mom, bool div, float fd,
                                              const SgdOp& op, int lane) {
  constexpr int kAux = 2;                            // loads: nt
  constexpr int kStAux = POL == kPolWt ? 16 : kAux;  // stores: sc1 (write-through) or nt
  constexpr int KV = 2, EPV = 4;
  constexpr int kHBytes = kBlock * U * 16, kWBytes = kHBytes * KV;
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const auto rh = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(half), 0, kHBytes,
                                                    0x00020000);
  const auto rp = __builtin_amdgcn_make_buffer_rsrc(par, 0, kWBytes, 0x00020000);
  const auto rm = __builtin_amdgcn_make_buffer_rsrc(mom, 0, kWBytes, 0x00020000);
  const int l = lane & 63, wave0 = lane & ~63;
  vec16 h[U], p[U][KV], m[U][KV];
#pragma unroll
  for (int j = 0; j < U; ++j) {
    h[j] = bitcast<vec16>(
        __builtin_amdgcn_raw_buffer_load_b128(rh, (j * kBlock + lane) * 16, 0, kAux));
#pragma unroll
    for (int v = 0; v < KV; ++v) {
      const int off = ((j * kBlock + wave0) * KV + v * 64 + l) * 16;
      p[j][v] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rp, off, 0, kAux));
      m[j][v] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rm, off, 0, kAux));
    }
  }
#pragma unroll
  for (int j = 0; j < U; ++j) {
#pragma unroll
    for (int v = 0; v < KV; ++v) {
      // as the decompress: output vector g of the wave holds sub-vector g % KV
      // of the unit lane g / KV loaded
      const int g = v * 64 + l;
      const int from = (g / KV) * 4, sub = g % KV;
      uint32_t w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        w[k] = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)h[j].w[k]);
      uint32_t d[EPV / 2];
#pragma unroll
      for (int k = 0; k < EPV / 2; ++k) {
        // both read before the select: a select between the two lvalues
        // becomes a dynamically indexed array, which lands in LDS
        const uint32_t lo = w[k], hi = w[EPV / 2 + k];
        d[k] = sub == 1 ? hi : lo;
      }
#pragma unroll
      for (int e = 0; e < EPV; ++e)
        sgd_elem<N>((uint16_t)(d[e >> 1] >> ((e & 1) * 16)), div, fd, op, p[j][v].w[e],
                    m[j][v].w[e]);
      const int off = ((j * kBlock + wave0) * KV + g) * 16;
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(p[j][v]), rp, off, 0, kStAux);
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(m[j][v]), rm, off, 0, kStAux);
    }
  }
}

// The partial tile: units [0, nunits) of the record; a unit past nunits is
// neither read nor written.
template <class N, int U>
__device__ __forceinline__ void sgd_tile_guarded(const unsigned char* half, unsigned char* par,
                                                 unsigned char* mom, uint64_t nunits, bool div,
                                                 float fd, const SgdOp& op, int lane) {
  constexpr int KV = 2;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const uint64_t u = (uint64_t)j * kBlock + lane;
    if (u >= nunits) continue;
    const vec16 h = ld16<true>(half + u * 16);
    vec16 p[KV], m[KV];
#pragma unroll
    for (int v = 0; v < KV; ++v) {
      p[v] = ld16<true>(par + (u * KV + v) * 16);
      m[v] = ld16<true>(mom + (u * KV + v) * 16);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
      sgd_elem<N>((uint16_t)(h.w[e >> 1] >> ((e & 1) * 16)), div, fd, op, p[e >> 2].w[e & 3],
                  m[e >> 2].w[e & 3]);
#pragma unroll
    for (int v = 0; v < KV; ++v) {
      st16<true>(par + (u * KV + v) * 16, p[v]);
      st16<true>(mom + (u * KV + v) * 16, m[v]);
    }
  }
}

// Elements [0, count), one per thread; `al` covers all three operands
// (cast_cut_ef).
template <class N>
__device__ __forceinline__ void sgd_elements(const unsigned char* half, unsigned char* par,
                                             unsigned char* mom, uint32_t count, bool al, bool div,
                                             float fd, const SgdOp& op, uint32_t t) {
  for (uint32_t e = t; e < count; e += kBlock) {
    uint32_t p = ld_e<uint32_t>(par + (uint64_t)e * 4, al);
    uint32_t m = ld_e<uint32_t>(mom + (uint64_t)e * 4, al);
    sgd_elem<N>(ld_e<uint16_t>(half + (uint64_t)e * 2, al), div, fd, op, p, m);
    st_e<uint32_t>(par + (uint64_t)e * 4, p, al);
    st_e<uint32_t>(mom + (uint64_t)e * 4, m, al);
  }
}

template <class N, int U, int POL>
__global__ __launch_bounds__(kBlock) void cast_sgd_kernel(SgdPlan a) {
  // The clip record, where there is one: wave-uniform (scalar) loads beside
  // the table record's.  A skipped step ends here, before any vector access.
  SgdOp op{a.lr, a.mu, a.wd, 1.0f, a.rec != nullptr, a.wd != 0.0f, a.nesterov != 0};
  if (a.rec) {
    const double nonfinite = a.rec->nonfinite;
    op.mult = a.rec->mult;
    if (a.skip && nonfinite != 0.0) return;
  }
  // grid == nrecords, as in cast_plan_kernel
  const CastRec& r = a.table[blockIdx.x];
  unsigned char* const par = r.wide;
  unsigned char* const half = r.half;
  unsigned char* const mom = a.mtab[blockIdx.x];
  const uint32_t kind = r.kind, count = r.count, aligned = r.aligned;
  asm volatile("" ::"s"(par), "s"(half), "s"(mom), "s"(kind), "s"(count), "s"(aligned));
  // the record prefetch of cast_plan_kernel, the third lane on the momentum
  // pointer's entry
  uint32_t pf = 0;
  if (threadIdx.x < 3 && blockIdx.x + kPrefetchAhead < a.nrecords) {
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(a.table + blockIdx.x + kPrefetchAhead);
    pf = *(threadIdx.x < 2
               ? rec + threadIdx.x * 7
               : reinterpret_cast<const uint32_t*>(a.mtab + blockIdx.x + kPrefetchAhead));
  }
  const bool div = a.divisor > 1;
  const float fd = (float)a.divisor;
  if (kind == kTileFull)
    sgd_tile_full<N, U, POL>(half, par, mom, div, fd, op, threadIdx.x);
  else if (kind == kTilePartial)
    sgd_tile_guarded<N, U>(half, par, mom, count, div, fd, op, threadIdx.x);
  else
    sgd_elements<N>(half, par, mom, count, aligned != 0, div, fd, op, threadIdx.x);
  keep_prefetch(pf);
}

// `u`: the tile size the table was cut for; `out_bytes`: what the launch
// writes, 8 an element (store policy, the decompress's rule).
template <class N>
static hipError_t launch_cast_plan_sgd_t(const SgdPlan& p, int u, uint64_t out_bytes,
                                         const Tuning& tu, hipStream_t s) {
  if (u != 1 && u != 2 && u != 4) return hipErrorInvalidValue;
  return cast_dispatch(u, cast_store_pol(tu, out_bytes), [&](auto U, auto POL) {
    return launch_cast_kernel<cast_sgd_kernel<N, decltype(U)::value, decltype(POL)::value>>(
        p, p.nrecords, tu.occ_min_tiles_batch, tu, s);
  });
}

}  // namespace bpsr
