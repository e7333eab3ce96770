// Top-k sparsification with error feedback: the kernels of bpsr_topk.h
// (the definition is prophet_amd/topk.py — one IEEE f32 add
// an element, then integers only).
//
//   ZERO        the plan's histograms
//   ACCUMULATE  c = g + r over r; histogram of key >> 20 (11 bits)
//   PICK d      per segment: the bin of digit d that holds the k-th largest
//               key, and how many elements are still wanted inside it
//   REFINE d    histogram of digit d (10 bits) among the keys that carry the
//               digits picked so far; a tile with no such key leaves at once
//   COUNT       per tile #{key > T} and #{key == T}
//   SCAN        per segment the exclusive sums of those over its tiles, and
//               the payload's header
//   COMPACT     sel per element, its slot, the indices, the values, r'
//   FOLD        out = (+0 + s_0 + ... + s_{N-1}) [/ divisor], sparse adds in LDS
//
// No workgroup waits on another: the order between passes is the stream's.
//
// The lane map is the cast tiles': a workgroup owns 4,096 contiguous elements,
// lane l's j-th b128 vector is vector j * 256 + l, so word [j][e] of a lane is
// element 4 (256 j + l) + e of the tile and ascending element order is (j,
// wave, lane, e).  COMPACT needs every selected element's rank in that order:
// a lane packs its vector's counts as #gt | #eq << 16 (a tile's totals fit 13
// bits), a wave prefix-sums the four packed words over its lanes (six
// ds_bpermute steps each), lane 63 leaves the wave's totals in LDS and every
// lane adds the 16 (j, wave) totals ahead of its own.  The slot of a selected
// element is gt_before + min(eq_before, need_eq), both counted over the whole
// segment: SCAN's tile sums plus the rank inside the tile.
//
// Histograms are one array of LDS words a workgroup (ds_add_u32), a lane adding
// its vector's equal bins once, flushed bin by bin — the non-zero ones — with
// global integer atomics: counts do not depend on the order.
//
// FOLD: a workgroup owns 4,096 outputs in LDS.  The two bounds of each source's
// index range inside the tile are 2 N lower-bound searches, dealt to the four
// waves and run in lockstep: a step probes 64 split points (one load a lane,
// one ballot) and keeps one 64th of the range.  Then source after source, in
// argument order and a barrier apart, lanes stride the range and add into LDS;
// the next source's entries are loaded ahead of this one's adds.
//
// The tile's loads, the histograms, the wave scan and FOLD's sparse sum are
// bpsr_topk_tile.h's: the server round's first pass (bpsr_k_topk_refold.hip)
// runs the same ones.
#include "bpsr_topk_tile.h"

namespace bpsr {

__global__ __launch_bounds__(kBlock) void topk_zero_kernel(TopKCompress p) {
  // grid == nsegs * kTopKBins / (4 kBlock): a b128 store a lane
  u4* const h = reinterpret_cast<u4*>(p.hist);
  h[(uint64_t)blockIdx.x * kBlock + threadIdx.x] = u4{0, 0, 0, 0};
}

template <int POL>
__global__ __launch_bounds__(kBlock) void topk_accum_kernel(TopKCompress p) {
  __shared__ uint32_t h[kDigitBins[0]];
  // grid == nrecs: no bounds test in front of the record load
  const TopKRec& r = p.recs[blockIdx.x];
  const unsigned char* const g = r.a;
  unsigned char* const q = r.b;
  const uint32_t seg = r.seg, count = r.count, flags = r.flags;
  asm volatile("" ::"s"(g), "s"(q), "s"(seg), "s"(count), "s"(flags));
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = lane; i < kDigitBins[0]; i += kBlock) h[i] = 0;
  auto add = [](uint32_t x, uint32_t y) {
    return bitcast<uint32_t>(bitcast<float>(x) + bitcast<float>(y));
  };
  uint32_t c[4][4];
  uint32_t valid = 0;
  if ((flags & kTopKVec) && count == kTopKTile) {
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
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) c[j][e] = y[j].w[e] = add(x[j].w[e], y[j].w[e]);
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(y[j]), rq, (int)vector_of(j, lane) * 16,
                                             0, kStAux<POL>);
    }
    valid = 0xffffu;
  } else {
    // a ragged or misaligned tile: an element past count is neither read nor written
    const bool vec = (flags & kTopKVec) != 0, al = (flags & kTopKAligned) != 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t p0 = vector_of(j, lane) * 4;
      if (vec && p0 + 4 <= count) {
        const vec16 x = ld16<true>(g + (uint64_t)p0 * 4);
        vec16 y = ld16<true>(q + (uint64_t)p0 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) c[j][e] = y.w[e] = add(x.w[e], y.w[e]);
        st16<false>(q + (uint64_t)p0 * 4, y);
        valid |= 0xfu << (4 * j);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          c[j][e] = 0;
          if (p0 + e >= count) continue;
          const uint64_t at = (uint64_t)(p0 + e) * 4;
          c[j][e] = add(ld_e<uint32_t>(g + at, al), ld_e<uint32_t>(q + at, al));
          st_e<uint32_t>(q + at, c[j][e], al);
          valid |= 1u << (4 * j + e);
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t b[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = (c[j][e] & kKeyMask) >> kDigitShift[0];
    hist_vector(h, b, (valid >> (4 * j)) & 0xfu);
  }
  __syncthreads();
  hist_flush<kDigitBins[0]>(h, p.hist + (uint64_t)seg * kTopKBins);
}

// One workgroup a segment, on the stream of the pass that filled digit D's
// histogram.  Lane t owns BINS / kBlock bins, the highest first: the lanes'
// sums are prefix-summed from the top, the one lane whose run crosses `need`
// walks its bins and leaves the digit and what is still wanted inside it.
template <int D>
__global__ __launch_bounds__(kBlock) void topk_pick_kernel(TopKCompress p) {
  constexpr uint32_t BINS = kDigitBins[D], PER = BINS / kBlock;
  __shared__ uint32_t sc[kBlock];
  const uint32_t seg = blockIdx.x;
  const uint32_t k = p.segs[seg].k;
  if (k == 0) return;  // an empty segment
  uint32_t need = k, prefix = 0;
  if (D > 0) {
    need = p.pick[seg].need;
    prefix = p.pick[seg].prefix;
  }
  const uint32_t* const gh = p.hist + (uint64_t)seg * kTopKBins + kDigitAt[D];
  const uint32_t t = threadIdx.x, top = BINS - 1 - t * PER;
  uint32_t cnt[PER], s = 0;
#pragma unroll
  for (uint32_t i = 0; i < PER; ++i) s += cnt[i] = gh[top - i];
  sc[t] = s;
  __syncthreads();
  for (uint32_t d = 1; d < kBlock; d <<= 1) {
    const uint32_t v = t >= d ? sc[t - d] : 0;
    __syncthreads();
    sc[t] += v;
    __syncthreads();
  }
  const uint32_t incl = sc[t];
  uint32_t above = incl - s;
  if (above < need && need <= incl) {
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) {
      if (need <= above + cnt[i]) {
        p.pick[seg] = TopKPick{(prefix << (D == 0 ? kTopKBits0 : D == 1 ? kTopKBits1 : kTopKBits2)) |
                                   (top - i),
                               need - above};
        break;
      }
      above += cnt[i];
    }
  }
}

template <int D>
__global__ __launch_bounds__(kBlock) void topk_refine_kernel(TopKCompress p) {
  __shared__ uint32_t h[kDigitBins[D]];
  const TopKRec& r = p.recs[blockIdx.x];
  const unsigned char* const q = r.b;
  const uint32_t seg = r.seg, count = r.count, flags = r.flags;
  const uint32_t prefix = p.pick[seg].prefix;
  asm volatile("" ::"s"(q), "s"(seg), "s"(count), "s"(flags), "s"(prefix));
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = lane; i < kDigitBins[D]; i += kBlock) h[i] = 0;
  uint32_t c[4][4];
  const uint32_t valid = load_tile(q, count, flags, lane, c);
  uint32_t match = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      match |= (((c[j][e] & kKeyMask) >> kDigitShift[D - 1]) == prefix ? 1u : 0u) << (4 * j + e);
  match &= valid;
  // no candidate in the tile: nothing to add (also the barrier behind the zeroing)
  if (!__syncthreads_or((int)match)) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t b[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      b[e] = ((c[j][e] & kKeyMask) >> kDigitShift[D]) & (kDigitBins[D] - 1);
    hist_vector(h, b, (match >> (4 * j)) & 0xfu);
  }
  __syncthreads();
  hist_flush<kDigitBins[D]>(h, p.hist + (uint64_t)seg * kTopKBins + kDigitAt[D]);
}

__global__ __launch_bounds__(kBlock) void topk_count_kernel(TopKCompress p) {
  __shared__ uint32_t wsum[kTopKWaves];
  const TopKRec& r = p.recs[blockIdx.x];
  const unsigned char* const q = r.b;
  const uint32_t seg = r.seg, count = r.count, flags = r.flags;
  const uint32_t T = p.pick[seg].prefix;
  asm volatile("" ::"s"(q), "s"(count), "s"(flags), "s"(T));
  const uint32_t lane = threadIdx.x;
  uint32_t c[4][4];
  const uint32_t valid = load_tile(q, count, flags, lane, c);
  uint32_t n = 0;  // #gt | #eq << 16: a wave's 1,024 elements fit
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t key = c[j][e] & kKeyMask;
      const bool in = (valid >> (4 * j + e)) & 1;
      n += (in && key > T ? 1u : 0u) + (in && key == T ? 0x10000u : 0u);
    }
  n = wave_scan(n);
  if ((lane & 63) == 63) wsum[lane >> 6] = n;
  __syncthreads();
  if (lane == 0) {
    uint32_t gt = 0, eq = 0;
    for (uint32_t w = 0; w < kTopKWaves; ++w) {
      gt += wsum[w] & 0xffffu;
      eq += wsum[w] >> 16;
    }
    p.count[blockIdx.x] = TopKCount{gt, eq};
  }
}

// One workgroup a segment: the exclusive sums of its tiles' counts, in tile
// order, 4 tiles a lane and kScanBlock lanes a round with the totals carried
// over; and the payload's header.
constexpr uint32_t kScanBlock = 1024, kScanPer = 4;
__global__ __launch_bounds__(kScanBlock) void topk_scan_kernel(TopKCompress p) {
  __shared__ uint32_t wg[kScanBlock / 64], we[kScanBlock / 64];
  const TopKSeg& sg = p.segs[blockIdx.x];
  unsigned char* const payload = sg.payload;
  const uint64_t nelem = sg.nelem;
  const uint32_t k = sg.k, nrecs = sg.nrecs;
  const TopKCount* const cnt = p.count + sg.rec_begin;
  TopKCount* const before = p.before + sg.rec_begin;
  const uint32_t t = threadIdx.x, w = t >> 6;
  if (t == 0 && payload) {
    vec16 hd;
    hd.w[0] = k;
    hd.w[1] = (uint32_t)nelem;
    hd.w[2] = (uint32_t)(nelem >> 32);
    hd.w[3] = 0;
    st16<false>(payload, hd);
  }
  uint32_t cg = 0, ce = 0;  // the rounds so far
  for (uint32_t base = 0; base < nrecs; base += kScanBlock * kScanPer) {
    const uint32_t i0 = base + t * kScanPer;
    TopKCount x[kScanPer];
    uint32_t sgt = 0, seq = 0;
#pragma unroll
    for (uint32_t a = 0; a < kScanPer; ++a) {
      x[a] = i0 + a < nrecs ? cnt[i0 + a] : TopKCount{0, 0};
      sgt += x[a].gt;
      seq += x[a].eq;
    }
    const uint32_t ig = wave_scan(sgt), ie = wave_scan(seq);
    if ((t & 63) == 63) {
      wg[w] = ig;
      we[w] = ie;
    }
    __syncthreads();
    uint32_t bg = cg, be = ce;
    for (uint32_t v = 0; v < kScanBlock / 64; ++v) {
      if (v < w) {
        bg += wg[v];
        be += we[v];
      }
      cg += wg[v];
      ce += we[v];
    }
    bg += ig - sgt;
    be += ie - seq;
#pragma unroll
    for (uint32_t a = 0; a < kScanPer; ++a) {
      if (i0 + a < nrecs) before[i0 + a] = TopKCount{bg, be};
      bg += x[a].gt;
      be += x[a].eq;
    }
    __syncthreads();
  }
}

template <int POL>
__global__ __launch_bounds__(kBlock) void topk_compact_kernel(TopKCompress p) {
  __shared__ uint32_t wtot[4][kTopKWaves];
  const TopKRec& r = p.recs[blockIdx.x];
  unsigned char* const q = r.b;
  const uint32_t seg = r.seg, e0 = r.e0, count = r.count, flags = r.flags;
  unsigned char* const payload = p.segs[seg].payload;
  const uint32_t k = p.segs[seg].k;
  const uint32_t T = p.pick[seg].prefix, need_eq = p.pick[seg].need;
  const TopKCount bf = p.before[blockIdx.x];
  asm volatile("" ::"s"(q), "s"(payload), "s"(e0), "s"(count), "s"(flags), "s"(k), "s"(T),
               "s"(need_eq));
  uint32_t* const idx = reinterpret_cast<uint32_t*>(payload + kTopKHeader);
  uint32_t* const val = idx + k;
  const uint32_t lane = threadIdx.x, w = lane >> 6;
  uint32_t c[4][4];
  const uint32_t valid = load_tile(q, count, flags, lane, c);
  uint32_t gt = 0, eq = 0;  // bit 4 j + e
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t key = c[j][e] & kKeyMask;
      gt |= (key > T ? 1u : 0u) << (4 * j + e);
      eq |= (key == T ? 1u : 0u) << (4 * j + e);
    }
  gt &= valid;
  eq &= valid;
  uint32_t own[4], incl[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    own[j] = (uint32_t)__builtin_popcount((gt >> (4 * j)) & 0xfu) |
             (uint32_t)__builtin_popcount((eq >> (4 * j)) & 0xfu) << 16;
    incl[j] = wave_scan(own[j]);
  }
  if ((lane & 63) == 63) {
#pragma unroll
    for (int j = 0; j < 4; ++j) wtot[j][w] = incl[j];
  }
  __syncthreads();
  uint32_t ahead = 0;  // of (j, wave) pairs before (0, w), then before (j, w)
  for (uint32_t v = 0; v < w; ++v) ahead += wtot[0][v];
  const bool vec = (flags & kTopKVec) != 0, al = (flags & kTopKAligned) != 0;
  const bool full = vec && count == kTopKTile;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t rank = ahead + incl[j] - own[j];
    uint32_t G = bf.gt + (rank & 0xffffu), E = bf.eq + (rank >> 16);
    const uint32_t p0 = vector_of(j, lane) * 4;
    uint32_t sel = 0;
    vec16 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool isgt = (gt >> (4 * j + e)) & 1, iseq = (eq >> (4 * j + e)) & 1;
      y.w[e] = c[j][e];
      if (isgt || (iseq && E < need_eq)) {
        const uint32_t slot = G + (E < need_eq ? E : need_eq);
        if (slot < k) {  // holds by construction; a store never leaves the payload
          idx[slot] = e0 + p0 + e;
          val[slot] = c[j][e];
        }
        y.w[e] = 0;
        sel |= 1u << e;
      }
      G += isgt ? 1u : 0u;
      E += iseq ? 1u : 0u;
    }
    // r' differs from c where an element left: only those vectors are written
    if (sel) {
      if (full) {
        const auto rq = __builtin_amdgcn_make_buffer_rsrc(q, 0, kTileBytes, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(y), rq, (int)p0 * 4, 0, kStAux<POL>);
      } else if (vec && p0 + 4 <= count) {
        st16<false>(q + (uint64_t)p0 * 4, y);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if ((sel >> e) & 1) st_e<uint32_t>(q + (uint64_t)(p0 + e) * 4, 0u, al);
      }
    }
    // the rest of row j, then the waves of row j + 1 ahead of this one
    if (j < 3) {
      for (uint32_t v = w; v < kTopKWaves; ++v) ahead += wtot[j][v];
      for (uint32_t v = 0; v < w; ++v) ahead += wtot[j + 1][v];
    }
  }
}

template <int POL>
__global__ __launch_bounds__(kBlock) void topk_fold_kernel(TopKFold p) {
  __shared__ __attribute__((aligned(16))) float tile[kTopKTile];
  __shared__ uint32_t bound[kTopKMaxSrcs][2];
  const TopKRec& r = p.recs[blockIdx.x];
  unsigned char* const out = r.a;
  const uint32_t seg = r.seg, t0 = r.e0, count = r.count, flags = r.flags;
  // sizes come from the plan, never from a header
  const uint32_t k = p.segs[seg].k;
  const int nsrc = p.nsrc;
  asm volatile("" ::"s"(out), "s"(seg), "s"(t0), "s"(count), "s"(flags), "s"(k), "s"(nsrc));
  const unsigned char* const* const row = p.srcs + (uint64_t)seg * (uint32_t)nsrc;
  const uint32_t tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  auto idx_of = [&](int s) { return reinterpret_cast<const uint32_t*>(row[s] + kTopKHeader); };
#pragma unroll
  for (int j = 0; j < 4; ++j)
    *reinterpret_cast<u4*>(&tile[vector_of(j, tid) * 4]) = u4{0, 0, 0, 0};
  tile_bounds(idx_of, nsrc, k, t0, count, l, w, bound);
  __syncthreads();
  tile_adds(idx_of, nsrc, k, t0, count, tid, bound, tile);
  const bool div = p.divisor > 1;
  const float fd = (float)p.divisor;
  const bool vec = (flags & kTopKVec) != 0, al = (flags & kTopKAligned) != 0;
  const bool full = vec && count == kTopKTile;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t p0 = vector_of(j, tid) * 4;
    vec16 o = bitcast<vec16>(*reinterpret_cast<const u4*>(&tile[p0]));
    if (div) {
#pragma unroll
      for (int e = 0; e < 4; ++e) o.w[e] = bitcast<uint32_t>(bitcast<float>(o.w[e]) / fd);
    }
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

// f(POL) with the store policy as a std::integral_constant.
template <class F>
static hipError_t topk_with_pol(int pol, F&& f) {
  return pol == kPolWt ? f(std::integral_constant<int, kPolWt>{})
                       : f(std::integral_constant<int, kPolNt>{});
}

// These kernels hold their histograms and tiles in static LDS: plain launches,
// no residency request on top.
#define TOPK_LAUNCH(kernel, grid, block, arg)                            \
  do {                                                                   \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, arg);      \
    const hipError_t e_ = hipGetLastError();                             \
    if (e_ != hipSuccess) return e_;                                     \
  } while (0)

// The ten launches; accum(POL): the second one, which leaves c over the
// residual and digit 0's histogram.
template <class Accum>
static hipError_t topk_select(const TopKCompress& p, uint64_t resid_bytes, const Tuning& tu,
                              hipStream_t s, Accum&& accum) {
  if (p.nsegs == 0) return hipSuccess;
  return topk_with_pol(cast_store_pol(tu, resid_bytes), [&](auto POL) -> hipError_t {
    constexpr int kPol = decltype(POL)::value;
    if (p.nrecs) {
      TOPK_LAUNCH(topk_zero_kernel, p.nsegs * (kTopKBins / (4 * kBlock)), kBlock, p);
      const hipError_t e = accum(POL);
      if (e != hipSuccess) return e;
      TOPK_LAUNCH(topk_pick_kernel<0>, p.nsegs, kBlock, p);
      TOPK_LAUNCH(topk_refine_kernel<1>, p.nrecs, kBlock, p);
      TOPK_LAUNCH(topk_pick_kernel<1>, p.nsegs, kBlock, p);
      TOPK_LAUNCH(topk_refine_kernel<2>, p.nrecs, kBlock, p);
      TOPK_LAUNCH(topk_pick_kernel<2>, p.nsegs, kBlock, p);
      TOPK_LAUNCH(topk_count_kernel, p.nrecs, kBlock, p);
    }
    TOPK_LAUNCH(topk_scan_kernel, p.nsegs, kScanBlock, p);  // the headers, empty segments' too
    if (p.nrecs) TOPK_LAUNCH(topk_compact_kernel<kPol>, p.nrecs, kBlock, p);
    return hipSuccess;
  });
}

hipError_t launch_topk_compress(const TopKCompress& p, uint64_t resid_bytes, const Tuning& tu,
                                hipStream_t s) {
  return topk_select(p, resid_bytes, tu, s, [&](auto POL) -> hipError_t {
    TOPK_LAUNCH(topk_accum_kernel<decltype(POL)::value>, p.nrecs, kBlock, p);
    return hipSuccess;
  });
}

hipError_t launch_topk_refold(const TopKRefold& p, uint64_t resid_bytes, const Tuning& tu,
                              hipStream_t s) {
  return topk_select(p.c, resid_bytes, tu, s, [&](auto POL) -> hipError_t {
    return launch_topk_refold_accum(p, decltype(POL)::value, s);
  });
}

hipError_t launch_topk_fold(const TopKFold& p, uint64_t out_bytes, const Tuning& tu,
                            hipStream_t s) {
  if (p.nrecs == 0) return hipSuccess;
  return topk_with_pol(cast_store_pol(tu, out_bytes), [&](auto POL) -> hipError_t {
    TOPK_LAUNCH(topk_fold_kernel<decltype(POL)::value>, p.nrecs, kBlock, p);
    return hipSuccess;
  });
}

#undef TOPK_LAUNCH

}  // namespace bpsr
