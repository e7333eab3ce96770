// 1-bit sign compression with error feedback, host side
// (byteps_reduce_onebit_*, include/bpsr/reduce.h): the operand checks, the three
// plans' tables (bpsr_onebit.h) and the C entry points.  Every check runs
// before the first HIP call of its entry: a refused call has touched nothing.
#include <algorithm>
#include <cstring>

#include "bpsr_api_internal.h"
#include "bpsr_onebit.h"

struct byteps_reduce_onebit_plan {
  bool fold = false;
  bool refold = false;
  int nsrc = 0;          // fold, refold
  uint32_t nrecs = 0, nsegs = 0;
  uint64_t nelem = 0;    // of all segments (store policy)
  // on the device: the records, then the segments (compress) or the rows of
  // source pointers (fold); the partials (compress); a refold plan is a
  // compress plan with the rows of source pointers beside it
  void* table = nullptr;
  void* side = nullptr;
  void* part = nullptr;
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
  out.push_back({b, b + (uintptr_t)bytes, seg});
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

uint32_t align_flags(const void* a, const void* b) {
  const uintptr_t x = (uintptr_t)a | (uintptr_t)b;
  return (x % 16 == 0 ? kOneBitVec : 0u) | (x % 4 == 0 ? kOneBitAligned : 0u);
}

// The records of one segment: `tile` elements each, the last one ragged.
void cut(std::vector<OneBitRec>& recs, unsigned char* a, unsigned char* b, uint64_t nelem,
         uint32_t seg, uint32_t tile) {
  const uint32_t flags = align_flags(a, b);
  for (uint64_t e = 0; e < nelem; e += tile)
    recs.push_back(OneBitRec{a ? a + e * 4 : nullptr, b ? b + e * 4 : nullptr, seg, (uint32_t)(e / 64),
                             (uint32_t)std::min<uint64_t>(tile, nelem - e), flags});
}

template <class T>
hipError_t upload(void** dev, const std::vector<T>& host) {
  if (host.empty()) return hipSuccess;
  const size_t bytes = host.size() * sizeof(T);
  const hipError_t e = hipMalloc(dev, bytes);
  return e == hipSuccess ? hipMemcpy(*dev, host.data(), bytes, hipMemcpyHostToDevice) : e;
}

hipError_t plan_free(byteps_reduce_onebit_plan* p) {
  hipError_t e = hipSuccess;
  for (void* q : {p->table, p->side, p->part, p->rows})
    if (q) {
      const hipError_t e2 = hipFree(q);
      if (e == hipSuccess) e = e2;
    }
  delete p;
  return e;
}

int check_payload(const void* payload, int seg) {
  if ((uintptr_t)payload % 16)
    return fail(BYTEPS_REDUCE_EARGS, "segment %d: payload is not 16-byte aligned", seg);
  return BYTEPS_REDUCE_OK;
}

int check_count(uint64_t nelem, int seg) {
  if (nelem > kOneBitMaxElems)
    return fail(BYTEPS_REDUCE_EARGS, "segment %d: more than 2^37 elements", seg);
  return BYTEPS_REDUCE_OK;
}

}  // namespace

}  // namespace bpsr

using namespace bpsr;

extern "C" {

uint64_t byteps_reduce_onebit_payload_bytes(uint64_t nelem) {
  return onebit_payload_bytes(nelem);
}

int byteps_reduce_onebit_plan_create(const byteps_onebit_desc* segs, int nsegs,
                                     byteps_reduce_onebit_plan** out) {
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null plan out-pointer");
  *out = nullptr;
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  std::vector<OneBitRec> recs;
  std::vector<OneBitSeg> stab((size_t)nsegs);
  std::vector<Range> ranges;
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_onebit_desc& d = segs[i];
    if (int rc = check_count(d.nelem, i)) return rc;
    if (d.nelem > 0 && (!d.grad || !d.resid || !d.payload))
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    if (int rc = check_payload(d.payload, i)) return rc;
    // an empty segment still gets its header where it names a payload
    bool ok = !d.payload || add_range(ranges, d.payload, onebit_payload_bytes(d.nelem), i);
    if (d.nelem > 0)
      ok = ok && add_range(ranges, d.grad, d.nelem * 4, i) &&
           add_range(ranges, d.resid, d.nelem * 4, i);
    if (!ok) return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    const size_t first = recs.size();
    cut(recs, static_cast<unsigned char*>(const_cast<void*>(d.grad)),
        static_cast<unsigned char*>(d.resid), d.nelem, (uint32_t)i, kOneBitTile);
    stab[(size_t)i] = OneBitSeg{static_cast<unsigned char*>(d.payload), d.nelem, (uint32_t)first,
                                (uint32_t)(recs.size() - first), 0};
    total += d.nelem;
    if (recs.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_onebit_plan();
  p->nrecs = (uint32_t)recs.size();
  p->nsegs = (uint32_t)nsegs;
  p->nelem = total;
  hipError_t e = upload(&p->table, recs);
  if (e == hipSuccess) e = upload(&p->side, stab);
  if (e == hipSuccess && p->nrecs)
    e = hipMalloc(&p->part, (size_t)p->nrecs * kOneBitWaves * sizeof(double));
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "onebit plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_onebit_plan_compress(byteps_reduce_onebit_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (p->fold)
    return fail(BYTEPS_REDUCE_EARGS,
                "compress on a fold plan (byteps_reduce_onebit_fold_plan_launch)");
  if (p->refold)
    return fail(BYTEPS_REDUCE_EARGS,
                "compress on a refold plan (byteps_reduce_onebit_refold_plan_launch)");
  const OneBitCompress a{static_cast<const OneBitRec*>(p->table),
                         static_cast<const OneBitSeg*>(p->side), static_cast<double*>(p->part),
                         p->nrecs, p->nsegs};
  // more than 4 sources: the process-wide tuning as it stands
  const hipError_t e =
      launch_onebit_compress(a, p->nelem * 4, launch_tuning_for_n(kOneBitMaxSrcs),
                             stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "onebit compress kernel launch");
}

int byteps_reduce_onebit_fold_plan_create(const byteps_onebit_fold_desc* segs, int nsegs, int nsrc,
                                          byteps_reduce_onebit_plan** out) {
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null plan out-pointer");
  *out = nullptr;
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  if (nsrc < 1 || nsrc > kOneBitMaxSrcs)
    return fail(BYTEPS_REDUCE_EARGS, "nsrc %d outside 1..%d", nsrc, kOneBitMaxSrcs);
  std::vector<OneBitRec> recs;
  std::vector<const unsigned char*> rows((size_t)nsegs * (size_t)nsrc, nullptr);
  std::vector<Range> ranges;
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_onebit_fold_desc& d = segs[i];
    if (int rc = check_count(d.nelem, i)) return rc;
    if (d.nelem == 0) continue;
    if (!d.out || !d.payloads) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    bool ok = add_range(ranges, d.out, d.nelem * 4, i);
    for (int k = 0; k < nsrc; ++k) {
      const void* pl = d.payloads[k];
      if (!pl) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null payload %d", i, k);
      if (int rc = check_payload(pl, i)) return rc;
      ok = ok && add_range(ranges, pl, onebit_payload_bytes(d.nelem), i);
      rows[(size_t)i * (size_t)nsrc + (size_t)k] = static_cast<const unsigned char*>(pl);
    }
    if (!ok) return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    cut(recs, static_cast<unsigned char*>(d.out), nullptr, d.nelem, (uint32_t)i, kOneBitTile);
    total += d.nelem;
    if (recs.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_onebit_plan();
  p->fold = true;
  p->nsrc = nsrc;
  p->nrecs = (uint32_t)recs.size();
  p->nsegs = (uint32_t)nsegs;
  p->nelem = total;
  hipError_t e = upload(&p->table, recs);
  if (e == hipSuccess) e = upload(&p->side, rows);
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "onebit fold plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_onebit_fold_plan_launch(byteps_reduce_onebit_plan* p, int divisor,
                                          void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (!p->fold)
    return fail(BYTEPS_REDUCE_EARGS, "fold launch on a %s plan",
                p->refold ? "refold" : "compress");
  if (divisor < 1) return fail(BYTEPS_REDUCE_EARGS, "divisor %d < 1", divisor);
  const OneBitFold a{static_cast<const OneBitRec*>(p->table),
                     static_cast<const unsigned char* const*>(p->side), p->nrecs, p->nsrc,
                     divisor};
  const hipError_t e = launch_onebit_fold(a, p->nelem * 4, launch_tuning_for_n(kOneBitMaxSrcs),
                                          stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "onebit fold kernel launch");
}

int byteps_reduce_onebit_refold_plan_create(const byteps_onebit_refold_desc* segs, int nsegs,
                                            int nsrc, byteps_reduce_onebit_plan** out) {
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null plan out-pointer");
  *out = nullptr;
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  if (nsrc < 1 || nsrc > kOneBitMaxSrcs)
    return fail(BYTEPS_REDUCE_EARGS, "nsrc %d outside 1..%d", nsrc, kOneBitMaxSrcs);
  std::vector<OneBitRec> recs;
  std::vector<OneBitSeg> stab((size_t)nsegs);
  std::vector<const unsigned char*> rows((size_t)nsegs * (size_t)nsrc, nullptr);
  std::vector<Range> ranges;
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_onebit_refold_desc& d = segs[i];
    if (int rc = check_count(d.nelem, i)) return rc;
    if (d.nelem > 0 && (!d.payloads || !d.resid || !d.out_payload))
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    if (int rc = check_payload(d.out_payload, i)) return rc;
    // an empty segment still gets its header where it names an output payload
    bool ok = !d.out_payload ||
              add_range(ranges, d.out_payload, onebit_payload_bytes(d.nelem), i);
    if (d.nelem > 0) {
      ok = ok && add_range(ranges, d.resid, d.nelem * 4, i);
      for (int k = 0; k < nsrc; ++k) {
        const void* pl = d.payloads[k];
        if (!pl) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null payload %d", i, k);
        if (int rc = check_payload(pl, i)) return rc;
        ok = ok && add_range(ranges, pl, onebit_payload_bytes(d.nelem), i);
        rows[(size_t)i * (size_t)nsrc + (size_t)k] = static_cast<const unsigned char*>(pl);
      }
    }
    if (!ok) return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    const size_t first = recs.size();
    cut(recs, nullptr, static_cast<unsigned char*>(d.resid), d.nelem, (uint32_t)i, kOneBitTile);
    stab[(size_t)i] = OneBitSeg{static_cast<unsigned char*>(d.out_payload), d.nelem,
                                (uint32_t)first, (uint32_t)(recs.size() - first), 0};
    total += d.nelem;
    if (recs.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_onebit_plan();
  p->refold = true;
  p->nsrc = nsrc;
  p->nrecs = (uint32_t)recs.size();
  p->nsegs = (uint32_t)nsegs;
  p->nelem = total;
  hipError_t e = upload(&p->table, recs);
  if (e == hipSuccess) e = upload(&p->side, stab);
  if (e == hipSuccess) e = upload(&p->rows, rows);
  if (e == hipSuccess && p->nrecs)
    e = hipMalloc(&p->part, (size_t)p->nrecs * kOneBitWaves * sizeof(double));
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "onebit refold plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_onebit_refold_plan_launch(byteps_reduce_onebit_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (!p->refold)
    return fail(BYTEPS_REDUCE_EARGS, "refold launch on a %s plan", p->fold ? "fold" : "compress");
  const OneBitRefold a{{static_cast<const OneBitRec*>(p->table),
                        static_cast<const OneBitSeg*>(p->side), static_cast<double*>(p->part),
                        p->nrecs, p->nsegs},
                       static_cast<const unsigned char* const*>(p->rows), p->nsrc};
  const hipError_t e = launch_onebit_refold(a, p->nelem * 4, launch_tuning_for_n(kOneBitMaxSrcs),
                                            stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "onebit refold kernel launch");
}

int byteps_reduce_onebit_plan_destroy(byteps_reduce_onebit_plan* p) {
  if (!p) return BYTEPS_REDUCE_OK;
  const hipError_t e = plan_free(p);
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "onebit plan free");
}

}  // extern "C"
