// The SGD step inside the decompress over the bf16 wire
// (byteps_reduce_cast_plan_apply_sgd): the plan launch of bpsr_cast_sgd.h,
// where the arithmetic and the tile's shape are described.  A bf16 quotient
// can be an f32 subnormal: the divide keeps it, as the decompress's does.
#include "bpsr_cast_sgd.h"

namespace bpsr {

hipError_t launch_cast_plan_sgd_bf16(const CastRec* table, unsigned char* const* mtab,
                                     uint32_t nrecords, int divisor, const byteps_sgd_hyper& h,
                                     const byteps_clip_record* rec, int skip, int u,
                                     uint64_t out_bytes, const Tuning& tu, hipStream_t s) {
  const SgdPlan p{table, mtab, nrecords, divisor, h.lr, h.momentum, h.weight_decay,
                  h.nesterov, rec, skip};
  return launch_cast_plan_sgd_t<NarrowBF16>(p, u, out_bytes, tu, s);
}

}  // namespace bpsr
