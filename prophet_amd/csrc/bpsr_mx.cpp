// Block-scaled 8- and 4-bit wires, host side (byteps_reduce_mx_*,
// include/bpsr/reduce.h): the operand checks, the plans' tables (bpsr_mx.h) and
// the C entry points — the error-feedback compress and the fold, and the
// stateless wires' compress and rotated fold (byteps_reduce_mx_sr_*,
// byteps_reduce_mx_rht_fold_*), and the error-feedback wires' server round
// (byteps_reduce_mx_refold_*, FLOAT32 alone: bpsr_k_mx_refold.hip).  A plan
// carries the element type of its gradients or outputs (the _typed creates):
// FLOAT32 runs bpsr_k_mx.hip and bpsr_k_mx_sr.hip, FLOAT16 and BFLOAT16 run
// bpsr_k_mx_half.hip.  Every check runs before the first HIP call of its entry:
// a refused call has touched nothing.
#include <algorithm>
#include <cstring>

#include "bpsr_api_internal.h"
#include "bpsr_mx.h"

struct byteps_reduce_mx_plan {
  // which launch takes it: _plan_compress, _fold_plan_launch, _sr_plan_compress,
  // _rht_fold_plan_launch, _refold_plan_launch
  enum Kind { kCompress, kFold, kSrCompress, kRhtFold, kRefold };
  Kind kind = kCompress;
  bool rotate = false;  // kSrCompress
  // of the gradient (compress) or the output (fold): FLOAT32, FLOAT16 or BFLOAT16
  int dtype = BYTEPS_REDUCE_FLOAT32;
  uint32_t bits = 0;
  int nsrc = 0;  // fold, refold
  uint32_t nrecs = 0;
  uint64_t nelem = 0;  // of all segments (store policy)
  // on the device: the records, the segments, the rows of source pointers (fold)
  void* table = nullptr;
  void* side = nullptr;
  void* rows = nullptr;
};

namespace bpsr {

namespace {

struct Range {
  uintptr_t begin, end;
  int seg;
};

// `bytes` at `p` as a range of segment `seg`; false where it wraps.
bool add_range(std::vector<Range>& out, const void* p, uint64_t bytes, int seg) {
  const uintptr_t b = (uintptr_t)p;
  if (bytes > UINTPTR_MAX - b) return false;
  if (bytes) out.push_back({b, b + (uintptr_t)bytes, seg});
  return true;
}

// All ranges pairwise disjoint (bpsr_cast_table.cpp's sweep).
int check_disjoint(std::vector<Range>& ranges) {
  std::sort(ranges.begin(), ranges.end(),
            [](const Range& a, const Range& b) { return a.begin < b.begin; });
  for (size_t k = 1, far = 0; k < ranges.size(); ++k) {
    if (ranges[k].begin < ranges[far].end)
      return fail(BYTEPS_REDUCE_EARGS, "segments %d and %d overlap", ranges[far].seg,
                  ranges[k].seg);
    if (ranges[k].end > ranges[far].end) far = k;
  }
  return BYTEPS_REDUCE_OK;
}

// The records of one segment: kMxTile elements each, contiguous and ascending,
// the last one ragged; `header`: an empty segment still gets one record.
// `esize`: the bytes of an element of `a`; `b` is f32.
void cut(std::vector<MxRec>& recs, unsigned char* a, unsigned char* b, uint64_t nelem,
         uint32_t seg, bool header, uint64_t esize) {
  const uintptr_t x = (uintptr_t)a | (uintptr_t)b;
  const uint32_t flags =
      esize == 4 ? (x % 16 == 0 ? kMxVec : 0u) | (x % 4 == 0 ? kMxAligned : 0u)
                 : ((uintptr_t)a % 16 == 0 ? kMxVec : 0u) | ((uintptr_t)b % 16 == 0 ? kMxVecB : 0u) |
                       kMxAligned;
  if (nelem == 0 && header) recs.push_back(MxRec{nullptr, nullptr, seg, 0, 0, flags});
  for (uint64_t e = 0; e < nelem; e += kMxTile)
    recs.push_back(MxRec{a + e * esize, b ? b + e * 4 : nullptr, seg, (uint32_t)e,
                         (uint32_t)std::min<uint64_t>(kMxTile, nelem - e), flags});
}

template <class T>
hipError_t upload(void** dev, const std::vector<T>& host) {
  if (host.empty()) return hipSuccess;
  const size_t bytes = host.size() * sizeof(T);
  const hipError_t e = hipMalloc(dev, bytes);
  return e == hipSuccess ? hipMemcpy(*dev, host.data(), bytes, hipMemcpyHostToDevice) : e;
}

hipError_t plan_free(byteps_reduce_mx_plan* p) {
  hipError_t e = hipSuccess;
  for (void* q : {p->table, p->side, p->rows})
    if (q) {
      const hipError_t e2 = hipFree(q);
      if (e == hipSuccess) e = e2;
    }
  delete p;
  return e;
}

// The bytes of an element of `dtype`, 0 for a type the wires do not take.
uint64_t mx_elem_size(int dtype) {
  return dtype == kFloat32 ? 4 : dtype == kFloat16 || dtype == kBFloat16 ? 2 : 0;
}

int check_table(const void* segs, int nsegs, int bits, int dtype, byteps_reduce_mx_plan** out) {
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null plan out-pointer");
  *out = nullptr;
  if (!mx_elem_size(dtype))
    return fail(BYTEPS_REDUCE_EDTYPE, "dtype %d: FLOAT32, FLOAT16 or BFLOAT16", dtype);
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  if (bits != 8 && bits != 4)
    return fail(BYTEPS_REDUCE_EARGS, "element bits %d: 8 (e4m3) or 4 (e2m1)", bits);
  return BYTEPS_REDUCE_OK;
}

// nelem of segment `seg`, and one operand's alignment.
int check_operand(uint64_t nelem, const void* p, unsigned align, const char* what, int seg) {
  if (nelem > kMxMaxElems)
    return fail(BYTEPS_REDUCE_EARGS, "segment %d: more than 2^31 elements", seg);
  if ((uintptr_t)p % align)
    return fail(BYTEPS_REDUCE_EARGS, "segment %d: %s is not %u-byte aligned", seg, what, align);
  return BYTEPS_REDUCE_OK;
}

}  // namespace

}  // namespace bpsr

using namespace bpsr;

extern "C" {

uint64_t byteps_reduce_mx_payload_bytes(uint64_t nelem, int bits) {
  return (bits == 8 || bits == 4) && nelem <= kMxMaxElems ? mx_payload_bytes(nelem, (uint32_t)bits)
                                                          : 0;
}

int byteps_reduce_mx_plan_create(const byteps_mx_desc* segs, int nsegs, int bits,
                                 byteps_reduce_mx_plan** out) {
  return byteps_reduce_mx_plan_create_typed(segs, nsegs, bits, BYTEPS_REDUCE_FLOAT32, out);
}

int byteps_reduce_mx_plan_create_typed(const byteps_mx_desc* segs, int nsegs, int bits,
                                       int dtype, byteps_reduce_mx_plan** out) {
  if (int rc = check_table(segs, nsegs, bits, dtype, out)) return rc;
  const uint64_t es = mx_elem_size(dtype);
  std::vector<MxRec> recs;
  std::vector<MxSeg> stab((size_t)nsegs);
  std::vector<Range> ranges;
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_mx_desc& d = segs[i];
    if (int rc = check_operand(d.nelem, d.payload, 16, "payload", i)) return rc;
    if (int rc = check_operand(d.nelem, d.grad, (unsigned)es, "gradient", i)) return rc;
    if (int rc = check_operand(d.nelem, d.resid, 4, "residual", i)) return rc;
    if (d.nelem > 0 && (!d.grad || !d.resid || !d.payload))
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    // an empty segment still gets its header where it names a payload
    bool ok = !d.payload ||
              add_range(ranges, d.payload, mx_payload_bytes(d.nelem, (uint32_t)bits), i);
    ok = ok && add_range(ranges, d.grad, d.nelem * es, i) &&
         add_range(ranges, d.resid, d.nelem * 4, i);
    if (!ok) return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    cut(recs, static_cast<unsigned char*>(const_cast<void*>(d.grad)),
        static_cast<unsigned char*>(d.resid), d.nelem, (uint32_t)i, d.payload != nullptr, es);
    stab[(size_t)i] = MxSeg{static_cast<unsigned char*>(d.payload), d.nelem};
    total += d.nelem;
    if (recs.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_mx_plan();
  p->dtype = dtype;
  p->bits = (uint32_t)bits;
  p->nrecs = (uint32_t)recs.size();
  p->nelem = total;
  hipError_t e = upload(&p->table, recs);
  if (e == hipSuccess) e = upload(&p->side, stab);
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "mx plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_mx_plan_compress(byteps_reduce_mx_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (p->kind != byteps_reduce_mx_plan::kCompress)
    return fail(BYTEPS_REDUCE_EARGS, "compress on a plan of another kind");
  const MxCompress a{static_cast<const MxRec*>(p->table), static_cast<const MxSeg*>(p->side),
                     p->nrecs};
  // more than 4 sources: the process-wide tuning as it stands
  const Tuning tu = launch_tuning_for_n(kMxMaxSrcs);
  const hipError_t e =
      p->dtype == kFloat32
          ? launch_mx_compress(a, p->bits, p->nelem * 4, tu, stream_of(stream))
          : launch_mx_half_compress(a, p->dtype, p->bits, p->nelem * 4, tu, stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "mx compress kernel launch");
}

int byteps_reduce_mx_fold_plan_create(const byteps_mx_fold_desc* segs, int nsegs, int nsrc,
                                      int bits, byteps_reduce_mx_plan** out) {
  return byteps_reduce_mx_fold_plan_create_typed(segs, nsegs, nsrc, bits, BYTEPS_REDUCE_FLOAT32,
                                                 out);
}

int byteps_reduce_mx_fold_plan_create_typed(const byteps_mx_fold_desc* segs, int nsegs, int nsrc,
                                            int bits, int dtype, byteps_reduce_mx_plan** out) {
  if (int rc = check_table(segs, nsegs, bits, dtype, out)) return rc;
  const uint64_t es = mx_elem_size(dtype);
  if (nsrc < 1 || nsrc > kMxMaxSrcs)
    return fail(BYTEPS_REDUCE_EARGS, "nsrc %d outside 1..%d", nsrc, kMxMaxSrcs);
  std::vector<MxRec> recs;
  std::vector<MxSeg> stab((size_t)nsegs);
  std::vector<const unsigned char*> rows((size_t)nsegs * (size_t)nsrc, nullptr);
  std::vector<Range> ranges;
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_mx_fold_desc& d = segs[i];
    if (int rc = check_operand(d.nelem, d.out, (unsigned)es, "output", i)) return rc;
    stab[(size_t)i] = MxSeg{nullptr, d.nelem};
    if (d.nelem == 0) continue;
    if (!d.out || !d.payloads) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    bool ok = add_range(ranges, d.out, d.nelem * es, i);
    for (int s = 0; s < nsrc; ++s) {
      const void* pl = d.payloads[s];
      if (!pl) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null payload %d", i, s);
      if (int rc = check_operand(d.nelem, pl, 16, "payload", i)) return rc;
      ok = ok && add_range(ranges, pl, mx_payload_bytes(d.nelem, (uint32_t)bits), i);
      rows[(size_t)i * (size_t)nsrc + (size_t)s] = static_cast<const unsigned char*>(pl);
    }
    if (!ok) return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    cut(recs, static_cast<unsigned char*>(d.out), nullptr, d.nelem, (uint32_t)i, false, es);
    total += d.nelem;
    if (recs.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_mx_plan();
  p->kind = byteps_reduce_mx_plan::kFold;
  p->dtype = dtype;
  p->bits = (uint32_t)bits;
  p->nsrc = nsrc;
  p->nrecs = (uint32_t)recs.size();
  p->nelem = total;
  hipError_t e = upload(&p->table, recs);
  if (e == hipSuccess) e = upload(&p->side, stab);
  if (e == hipSuccess) e = upload(&p->rows, rows);
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "mx fold plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_mx_fold_plan_launch(byteps_reduce_mx_plan* p, int divisor, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (p->kind != byteps_reduce_mx_plan::kFold)
    return fail(BYTEPS_REDUCE_EARGS, "fold launch on a plan of another kind");
  if (divisor < 1) return fail(BYTEPS_REDUCE_EARGS, "divisor %d < 1", divisor);
  const MxFold a{static_cast<const MxRec*>(p->table),
                 static_cast<const MxSeg*>(p->side),
                 static_cast<const unsigned char* const*>(p->rows),
                 p->nrecs,
                 p->nsrc,
                 divisor};
  const Tuning tu = launch_tuning_for_n(kMxMaxSrcs);
  const hipError_t e =
      p->dtype == kFloat32
          ? launch_mx_fold(a, p->bits, p->nelem * 4, tu, stream_of(stream))
          : launch_mx_half_fold(a, p->dtype, p->bits, p->nelem * 2, tu, stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "mx fold kernel launch");
}

int byteps_reduce_mx_refold_plan_create(const byteps_mx_refold_desc* segs, int nsegs, int nsrc,
                                        int bits, byteps_reduce_mx_plan** out) {
  if (int rc = check_table(segs, nsegs, bits, BYTEPS_REDUCE_FLOAT32, out)) return rc;
  if (nsrc < 1 || nsrc > kMxMaxSrcs)
    return fail(BYTEPS_REDUCE_EARGS, "nsrc %d outside 1..%d", nsrc, kMxMaxSrcs);
  std::vector<MxRec> recs;
  std::vector<MxSeg> stab((size_t)nsegs);
  std::vector<const unsigned char*> rows((size_t)nsegs * (size_t)nsrc, nullptr);
  std::vector<Range> ranges;
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_mx_refold_desc& d = segs[i];
    if (int rc = check_operand(d.nelem, d.out, 16, "output payload", i)) return rc;
    if (int rc = check_operand(d.nelem, d.resid, 4, "residual", i)) return rc;
    if (d.nelem > 0 && (!d.resid || !d.out || !d.srcs))
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    // an empty segment still gets its header where it names an output payload
    bool ok = (!d.out || add_range(ranges, d.out, mx_payload_bytes(d.nelem, (uint32_t)bits), i)) &&
              add_range(ranges, d.resid, d.nelem * 4, i);
    for (int s = 0; d.nelem > 0 && s < nsrc; ++s) {
      const void* pl = d.srcs[s];
      if (!pl) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null payload %d", i, s);
      if (int rc = check_operand(d.nelem, pl, 16, "payload", i)) return rc;
      ok = ok && add_range(ranges, pl, mx_payload_bytes(d.nelem, (uint32_t)bits), i);
      rows[(size_t)i * (size_t)nsrc + (size_t)s] = static_cast<const unsigned char*>(pl);
    }
    if (!ok) return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    cut(recs, static_cast<unsigned char*>(d.resid), nullptr, d.nelem, (uint32_t)i,
        d.out != nullptr, 4);
    stab[(size_t)i] = MxSeg{static_cast<unsigned char*>(d.out), d.nelem};
    total += d.nelem;
    if (recs.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  // the output payload aliases no source and no residual; sources are distinct
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_mx_plan();
  p->kind = byteps_reduce_mx_plan::kRefold;
  p->bits = (uint32_t)bits;
  p->nsrc = nsrc;
  p->nrecs = (uint32_t)recs.size();
  p->nelem = total;
  hipError_t e = upload(&p->table, recs);
  if (e == hipSuccess) e = upload(&p->side, stab);
  if (e == hipSuccess) e = upload(&p->rows, rows);
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "mx refold plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_mx_refold_plan_launch(byteps_reduce_mx_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (p->kind != byteps_reduce_mx_plan::kRefold)
    return fail(BYTEPS_REDUCE_EARGS, "refold launch on a plan of another kind");
  const MxRefold a{static_cast<const MxRec*>(p->table), static_cast<const MxSeg*>(p->side),
                   static_cast<const unsigned char* const*>(p->rows), p->nrecs, p->nsrc};
  const Tuning tu = launch_tuning_for_n(kMxMaxSrcs);
  const hipError_t e = launch_mx_refold(a, p->bits, p->nelem * 4, tu, stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "mx refold kernel launch");
}

int byteps_reduce_mx_sr_plan_create(const byteps_mx_sr_desc* segs, int nsegs, int bits,
                                    int rotate, byteps_reduce_mx_plan** out) {
  return byteps_reduce_mx_sr_plan_create_typed(segs, nsegs, bits, rotate, BYTEPS_REDUCE_FLOAT32,
                                               out);
}

int byteps_reduce_mx_sr_plan_create_typed(const byteps_mx_sr_desc* segs, int nsegs, int bits,
                                          int rotate, int dtype, byteps_reduce_mx_plan** out) {
  if (int rc = check_table(segs, nsegs, bits, dtype, out)) return rc;
  const uint64_t es = mx_elem_size(dtype);
  if (rotate != 0 && rotate != 1) return fail(BYTEPS_REDUCE_EARGS, "rotate %d: 0 or 1", rotate);
  std::vector<MxRec> recs;
  std::vector<MxSrSeg> stab((size_t)nsegs);
  std::vector<Range> ranges;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_mx_sr_desc& d = segs[i];
    if (int rc = check_operand(d.nelem, d.payload, 16, "payload", i)) return rc;
    if (int rc = check_operand(d.nelem, d.grad, (unsigned)es, "gradient", i)) return rc;
    if (d.nelem > 0 && (!d.grad || !d.payload))
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    // an empty segment still gets its header where it names a payload
    const bool ok = (!d.payload ||
                     add_range(ranges, d.payload, mx_payload_bytes(d.nelem, (uint32_t)bits), i)) &&
                    add_range(ranges, d.grad, d.nelem * es, i);
    if (!ok) return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    cut(recs, static_cast<unsigned char*>(const_cast<void*>(d.grad)), nullptr, d.nelem,
        (uint32_t)i, d.payload != nullptr, es);
    stab[(size_t)i] = MxSrSeg{static_cast<unsigned char*>(d.payload), d.nelem, d.key, d.rot_key,
                              {0, 0}};
    if (recs.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_mx_plan();
  p->kind = byteps_reduce_mx_plan::kSrCompress;
  p->dtype = dtype;
  p->rotate = rotate == 1;
  p->bits = (uint32_t)bits;
  p->nrecs = (uint32_t)recs.size();
  hipError_t e = upload(&p->table, recs);
  if (e == hipSuccess) e = upload(&p->side, stab);
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "mx sr plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_mx_sr_plan_compress(byteps_reduce_mx_plan* p, uint32_t step, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (p->kind != byteps_reduce_mx_plan::kSrCompress)
    return fail(BYTEPS_REDUCE_EARGS, "stochastic compress on a plan of another kind");
  const MxSrCompress a{static_cast<const MxRec*>(p->table), static_cast<const MxSrSeg*>(p->side),
                       p->nrecs, step};
  const hipError_t e =
      p->dtype == kFloat32
          ? launch_mx_sr_compress(a, p->bits, p->rotate, stream_of(stream))
          : launch_mx_half_sr_compress(a, p->dtype, p->bits, p->rotate, stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "mx sr compress kernel launch");
}

int byteps_reduce_mx_rht_fold_plan_create(const byteps_mx_rht_fold_desc* segs, int nsegs,
                                          int nsrc, int bits, byteps_reduce_mx_plan** out) {
  return byteps_reduce_mx_rht_fold_plan_create_typed(segs, nsegs, nsrc, bits,
                                                     BYTEPS_REDUCE_FLOAT32, out);
}

int byteps_reduce_mx_rht_fold_plan_create_typed(const byteps_mx_rht_fold_desc* segs, int nsegs,
                                                int nsrc, int bits, int dtype,
                                                byteps_reduce_mx_plan** out) {
  if (int rc = check_table(segs, nsegs, bits, dtype, out)) return rc;
  const uint64_t es = mx_elem_size(dtype);
  if (nsrc < 1 || nsrc > kMxMaxSrcs)
    return fail(BYTEPS_REDUCE_EARGS, "nsrc %d outside 1..%d", nsrc, kMxMaxSrcs);
  std::vector<MxRec> recs;
  std::vector<MxSrSeg> stab((size_t)nsegs);
  std::vector<const unsigned char*> rows((size_t)nsegs * (size_t)nsrc, nullptr);
  std::vector<Range> ranges;
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_mx_rht_fold_desc& d = segs[i];
    if (int rc = check_operand(d.nelem, d.out, (unsigned)es, "output", i)) return rc;
    stab[(size_t)i] = MxSrSeg{nullptr, d.nelem, 0, d.rot_key, {0, 0}};
    if (d.nelem == 0) continue;
    if (!d.out || !d.payloads) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    bool ok = add_range(ranges, d.out, d.nelem * es, i);
    for (int s = 0; s < nsrc; ++s) {
      const void* pl = d.payloads[s];
      if (!pl) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null payload %d", i, s);
      if (int rc = check_operand(d.nelem, pl, 16, "payload", i)) return rc;
      ok = ok && add_range(ranges, pl, mx_payload_bytes(d.nelem, (uint32_t)bits), i);
      rows[(size_t)i * (size_t)nsrc + (size_t)s] = static_cast<const unsigned char*>(pl);
    }
    if (!ok) return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    cut(recs, static_cast<unsigned char*>(d.out), nullptr, d.nelem, (uint32_t)i, false, es);
    total += d.nelem;
    if (recs.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_mx_plan();
  p->kind = byteps_reduce_mx_plan::kRhtFold;
  p->dtype = dtype;
  p->bits = (uint32_t)bits;
  p->nsrc = nsrc;
  p->nrecs = (uint32_t)recs.size();
  p->nelem = total;
  hipError_t e = upload(&p->table, recs);
  if (e == hipSuccess) e = upload(&p->side, stab);
  if (e == hipSuccess) e = upload(&p->rows, rows);
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "mx rht fold plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_mx_rht_fold_plan_launch(byteps_reduce_mx_plan* p, int divisor, uint32_t step,
                                          void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (p->kind != byteps_reduce_mx_plan::kRhtFold)
    return fail(BYTEPS_REDUCE_EARGS, "rotated fold launch on a plan of another kind");
  if (divisor < 1) return fail(BYTEPS_REDUCE_EARGS, "divisor %d < 1", divisor);
  const MxRhtFold a{static_cast<const MxRec*>(p->table),
                    static_cast<const MxSrSeg*>(p->side),
                    static_cast<const unsigned char* const*>(p->rows),
                    p->nrecs,
                    p->nsrc,
                    divisor,
                    step};
  const Tuning tu = launch_tuning_for_n(kMxMaxSrcs);
  const hipError_t e =
      p->dtype == kFloat32
          ? launch_mx_rht_fold(a, p->bits, p->nelem * 4, tu, stream_of(stream))
          : launch_mx_half_rht_fold(a, p->dtype, p->bits, p->nelem * 2, tu, stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "mx rht fold kernel launch");
}

int byteps_reduce_mx_plan_destroy(byteps_reduce_mx_plan* p) {
  if (!p) return BYTEPS_REDUCE_OK;
  const hipError_t e = plan_free(p);
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "mx plan free");
}

}  // extern "C"
