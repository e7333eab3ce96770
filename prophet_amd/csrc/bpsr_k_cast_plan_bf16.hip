// Cast plan over the bf16 wire: bpsr_k_cast_plan.hip's kernel
// (bpsr_cast_plan.h) with the narrow format of bpsr_k_cast_bf16.hip, so every
// segment's bytes equal what the one-tensor bf16 call writes.  The table is
// the fp16 plan's: the narrow side is 2 bytes either way.
#include "bpsr_cast_plan.h"

namespace bpsr {

hipError_t launch_cast_plan_bf16(bool compress, const CastRec* table, uint32_t nrecords,
                                 int wide_dtype, int divisor, int u, uint64_t out_bytes,
                                 const Tuning& tu, hipStream_t s) {
  return launch_plan<NarrowBF16, kFloat16>(compress, table, nrecords, wide_dtype, divisor, u,
                                           out_bytes, tu, s);
}

hipError_t launch_cast_plan_stats_bf16(const CastRec* table, uint32_t nrecords, int wide_dtype,
                                       int divisor, int u, uint64_t out_bytes, void* part,
                                       const Tuning& tu, hipStream_t s) {
  return launch_plan_stats<NarrowBF16, kFloat16>(table, nrecords, wide_dtype, divisor, u,
                                                 out_bytes, static_cast<StatPart*>(part), tu, s);
}

hipError_t launch_cast_plan_measure_bf16(const CastRec* table, uint32_t nrecords, int wide_dtype,
                                         int divisor, int u, void* part, const Tuning& tu,
                                         hipStream_t s) {
  return launch_plan_measure<NarrowBF16, kFloat16>(table, nrecords, wide_dtype, divisor, u,
                                                   static_cast<StatPart*>(part), tu, s);
}

hipError_t launch_cast_plan_scaled_bf16(const CastRec* table, uint32_t nrecords, int wide_dtype,
                                        int divisor, int u, uint64_t out_bytes,
                                        const float* mult, const Tuning& tu, hipStream_t s) {
  return launch_plan_scaled<NarrowBF16, kFloat16>(table, nrecords, wide_dtype, divisor, u,
                                                  out_bytes, mult, tu, s);
}

}  // namespace bpsr
