// Error-feedback compress over the bf16 wire (Compression.bf16_ef):
// bpsr_k_cast_ef.hip's launches with the narrow format of bpsr_k_cast_bf16.hip.
// The bf16 wire keeps 8 significant bits an element; the other 16 stay in the
// residual instead of being dropped each step.
#include "bpsr_cast_ef.h"

namespace bpsr {

hipError_t launch_compress_ef_bf16(void* dst, void* resid, const void* src, size_t nelem,
                                   const Tuning& tu, hipStream_t s) {
  return launch_compress_ef_t<NarrowBF16>(dst, resid, src, nelem, tu, s);
}

hipError_t launch_cast_plan_ef_bf16(const CastRec* table, unsigned char* const* rtab,
                                    uint32_t nrecords, int u, uint64_t out_bytes,
                                    const Tuning& tu, hipStream_t s) {
  return launch_cast_plan_ef_t<NarrowBF16>(table, rtab, nrecords, u, out_bytes, tu, s);
}

}  // namespace bpsr
