// Cast plan (byteps_reduce_cast_plan_*): a whole iteration's fp16 casts in one
// launch.  A push_pull iteration compresses every gradient before the pushes
// and decompresses every result after the pulls; one cast_kernel launch per
// tensor (bpsr_k_cast.hip) is all launch cost for a model whose gradients are
// mostly a few KiB.  Here the segments are cut ahead of time into a resident
// table of CastRec records (bpsr_cast_table.cpp), one per workgroup, and
// workgroup b runs record b with the single cast's own per-tile code
// (bpsr_cast_impl.h), so every segment's bytes equal what the one-tensor call
// writes.
//
// The record is 32 bytes read at a wave-uniform address before anything is
// stored: scalar loads, one round trip, and both pointers arrive already
// advanced to the tile.  A full tile builds its two buffer descriptors from
// those scalars, sized to the tile — the hardware drops any access outside it —
// and the guarded tile and the element range read nothing past `count`.  The
// same table serves both directions (the record names the wide and the fp16
// side, COMPRESS picks which is read), and the divisor is a kernel argument:
// one plan, every divisor.  The kernel and its launch are templates on the wire
// format (bpsr_cast_plan.h); this unit instantiates the fp16 wire.
#include "bpsr_cast_plan.h"

namespace bpsr {

hipError_t launch_cast_plan(bool compress, const CastRec* table, uint32_t nrecords,
                            int wide_dtype, int divisor, int u, uint64_t out_bytes,
                            const Tuning& tu, hipStream_t s) {
  return launch_plan<NarrowF16, kBFloat16>(compress, table, nrecords, wide_dtype, divisor, u,
                                           out_bytes, tu, s);
}

hipError_t launch_cast_plan_stats(const CastRec* table, uint32_t nrecords, int wide_dtype,
                                  int divisor, int u, uint64_t out_bytes, void* part,
                                  const Tuning& tu, hipStream_t s) {
  return launch_plan_stats<NarrowF16, kBFloat16>(table, nrecords, wide_dtype, divisor, u,
                                                 out_bytes, static_cast<StatPart*>(part), tu, s);
}

hipError_t launch_cast_plan_measure(const CastRec* table, uint32_t nrecords, int wide_dtype,
                                    int divisor, int u, void* part, const Tuning& tu,
                                    hipStream_t s) {
  return launch_plan_measure<NarrowF16, kBFloat16>(table, nrecords, wide_dtype, divisor, u,
                                                   static_cast<StatPart*>(part), tu, s);
}

hipError_t launch_cast_plan_scaled(const CastRec* table, uint32_t nrecords, int wide_dtype,
                                   int divisor, int u, uint64_t out_bytes,
                                   const float* mult, const Tuning& tu, hipStream_t s) {
  return launch_plan_scaled<NarrowF16, kBFloat16>(table, nrecords, wide_dtype, divisor, u,
                                                  out_bytes, mult, tu, s);
}

// Finishes the statistics, one workgroup per segment, on the stream of the
// decompress (the kernel boundary makes every XCD's partials visible).  The
// segment's records — seg_recs[seg_begin[s] .. seg_begin[s + 1]), ascending —
// are dealt to the lanes in that order, lane t taking records t, t +
// kFinishBlock, ...; a lane adds its records' partials as they come, ascending
// record then wave; the waves add their lanes up (stat_wave_sum) and lane 0 the
// waves, in wave order.  The order depends on the plan alone.  Every row is
// written: a segment without records (nelem == 0) gets {0, 0}.
// One segment can own most of a plan's records (a 64 Mi-element tensor: 16 Ki
// records, 1 MiB of partials), and a record costs two dependent round trips —
// its index, then its 64 bytes of partials — to memory another XCD wrote.  One
// entry at a time on 256 lanes that was 0.16 ms against the decompress's 0.07
// (kernel trace).  So 1024 lanes; each loads kFinishIdx record
// indices at once, then the partials of kFinishAhead records at once.
constexpr uint32_t kFinishBlock = 1024, kFinishIdx = 16, kFinishAhead = 4;
__global__ __launch_bounds__(kFinishBlock) void cast_stats_finish_kernel(
    const uint32_t* __restrict__ seg_begin, const uint32_t* __restrict__ seg_recs,
    const StatPart* __restrict__ part, double* __restrict__ stats) {
  constexpr uint32_t kWaves = kBlock / 64;  // partials a record
  constexpr uint32_t kFinishWaves = kFinishBlock / 64;
  __shared__ double wsum[kFinishWaves];
  __shared__ uint64_t wcnt[kFinishWaves];
  const uint32_t s = blockIdx.x, b = seg_begin[s], n = seg_begin[s + 1] - b;
  double sum = 0.0;
  uint64_t cnt = 0;
  for (uint32_t r0 = threadIdx.x; r0 < n; r0 += kFinishBlock * kFinishIdx) {
    // n < 2^31 (build_cast_table) and r0 < n: r0 + a * kFinishBlock < 2^32
    uint32_t rec[kFinishIdx];
#pragma unroll
    for (uint32_t a = 0; a < kFinishIdx; ++a) {
      const uint32_t r = r0 + a * kFinishBlock;
      rec[a] = r < n ? seg_recs[b + r] : 0;
    }
#pragma unroll
    for (uint32_t a0 = 0; a0 < kFinishIdx; a0 += kFinishAhead) {
      StatPart q[kFinishAhead][kWaves];
#pragma unroll
      for (uint32_t a = 0; a < kFinishAhead; ++a)
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w)
          q[a][w] = r0 + (a0 + a) * kFinishBlock < n ? part[(uint64_t)rec[a0 + a] * kWaves + w]
                                                     : StatPart{0.0, 0};
#pragma unroll
      for (uint32_t a = 0; a < kFinishAhead; ++a)
        if (r0 + (a0 + a) * kFinishBlock < n) {
#pragma unroll
          for (uint32_t w = 0; w < kWaves; ++w) {
            sum += q[a][w].sumsq;
            cnt += q[a][w].nonfinite;
          }
        }
    }
  }
  stat_wave_sum(sum, cnt);
  if ((threadIdx.x & 63) == 0) {
    wsum[threadIdx.x >> 6] = sum;
    wcnt[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = wsum[0];
    uint64_t c = wcnt[0];
    for (uint32_t w = 1; w < kFinishWaves; ++w) {
      total += wsum[w];
      c += wcnt[w];
    }
    stats[2 * (uint64_t)s] = total;
    stats[2 * (uint64_t)s + 1] = (double)c;
  }
}

hipError_t launch_cast_stats_finish(const uint32_t* seg_begin, const uint32_t* seg_recs,
                                    const void* part, double* stats, int nsegs, hipStream_t s) {
  if (nsegs <= 0) return hipSuccess;
  hipLaunchKernelGGL(cast_stats_finish_kernel, dim3((uint32_t)nsegs), dim3(kFinishBlock), 0, s,
                     seg_begin, seg_recs, static_cast<const StatPart*>(part), stats);
  return hipGetLastError();
}

// The clip record (byteps_reduce_clip_record): one workgroup
// adds up `nrows` statistics rows — lane t takes rows t, t + kFinishBlock, ...
// in ascending order, the waves add their lanes up (stat_wave_sum) and lane 0
// the waves, in wave order: an order nrows alone fixes — and lane 0 derives
// the norm and the two multipliers in f64.  A row's count is an integer below
// 2^53 held in a double: added as integers, it stays exact.
__global__ __launch_bounds__(kFinishBlock) void clip_record_kernel(
    const double* __restrict__ rows, int nrows, double max_norm, double eps,
    const float* __restrict__ inv_scale, byteps_clip_record* __restrict__ out) {
  constexpr uint32_t kFinishWaves = kFinishBlock / 64;
  __shared__ double wsum[kFinishWaves];
  __shared__ uint64_t wcnt[kFinishWaves];
  double sum = 0.0;
  uint64_t cnt = 0;
  for (uint32_t r = threadIdx.x; r < (uint32_t)nrows; r += kFinishBlock) {
    sum += rows[2 * (uint64_t)r];
    cnt += (uint64_t)rows[2 * (uint64_t)r + 1];
  }
  stat_wave_sum(sum, cnt);
  if ((threadIdx.x & 63) == 0) {
    wsum[threadIdx.x >> 6] = sum;
    wcnt[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = wsum[0];
    uint64_t c = wcnt[0];
    for (uint32_t w = 1; w < kFinishWaves; ++w) {
      total += wsum[w];
      c += wcnt[w];
    }
    const double inv = inv_scale ? (double)*inv_scale : 1.0;
    const double norm = __builtin_sqrt(total) * inv;
    const double q = max_norm / (norm + eps);
    const double coef = q < 1.0 ? q : 1.0;
    out->sumsq = total;
    out->nonfinite = (double)c;
    out->norm = norm;
    out->coef = (float)coef;
    out->mult = (float)(coef * inv);
  }
}

hipError_t launch_clip_record(const double* rows, int nrows, double max_norm, double eps,
                              const float* inv_scale, byteps_clip_record* out, hipStream_t s) {
  hipLaunchKernelGGL(clip_record_kernel, dim3(1), dim3(kFinishBlock), 0, s, rows, nrows, max_norm,
                     eps, inv_scale, out);
  return hipGetLastError();
}

}  // namespace bpsr
