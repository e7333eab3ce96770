// Top-k sparsification with error feedback, host side (byteps_reduce_topk_*,
// include/bpsr/reduce.h): the operand checks, the three plans' tables and scratch
// (bpsr_topk.h) and the C entry points.  Every check runs before the first HIP
// call of its entry: a refused call has touched nothing.
#include <algorithm>
#include <cstring>

#include "bpsr_api_internal.h"
#include "bpsr_topk.h"

struct byteps_reduce_topk_plan {
  bool fold = false;
  bool refold = false;  // a compress plan whose gradient is the fold of `rows`
  int nsrc = 0;         // fold, refold
  uint32_t nrecs = 0, nsegs = 0;
  uint64_t nelem = 0;  // of all segments (store policy)
  // on the device: the records, the segments, the rows of source pointers
  // (fold, refold); the compress's scratch — histograms, pick state, the tiles' counts
  // and their sums
  void* table = nullptr;
  void* side = nullptr;
  void* rows = nullptr;
  void* hist = nullptr;
  void* pick = nullptr;
  void* count = nullptr;
  void* before = nullptr;
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

// The records of one segment: kTopKTile elements each, contiguous and
// ascending, the last one ragged.
void cut(std::vector<TopKRec>& recs, unsigned char* a, unsigned char* b, uint64_t nelem,
         uint32_t seg) {
  const uintptr_t x = (uintptr_t)a | (uintptr_t)b;
  const uint32_t flags = (x % 16 == 0 ? kTopKVec : 0u) | (x % 4 == 0 ? kTopKAligned : 0u);
  for (uint64_t e = 0; e < nelem; e += kTopKTile)
    recs.push_back(TopKRec{a + e * 4, b ? b + e * 4 : nullptr, seg, (uint32_t)e,
                           (uint32_t)std::min<uint64_t>(kTopKTile, nelem - e), flags});
}

template <class T>
hipError_t upload(void** dev, const std::vector<T>& host) {
  if (host.empty()) return hipSuccess;
  const size_t bytes = host.size() * sizeof(T);
  const hipError_t e = hipMalloc(dev, bytes);
  return e == hipSuccess ? hipMemcpy(*dev, host.data(), bytes, hipMemcpyHostToDevice) : e;
}

hipError_t plan_free(byteps_reduce_topk_plan* p) {
  hipError_t e = hipSuccess;
  for (void* q : {p->table, p->side, p->rows, p->hist, p->pick, p->count, p->before})
    if (q) {
      const hipError_t e2 = hipFree(q);
      if (e == hipSuccess) e = e2;
    }
  delete p;
  return e;
}

// nelem and k of segment `seg`, and its payload's alignment.
int check_sizes(uint64_t nelem, uint64_t k, const void* payload, int seg) {
  if (nelem > kTopKMaxElems)
    return fail(BYTEPS_REDUCE_EARGS, "segment %d: more than 2^31 elements", seg);
  if (nelem == 0 ? k != 0 : (k < 1 || k > nelem))
    return fail(BYTEPS_REDUCE_EARGS, "segment %d: k %llu outside 1..%llu", seg,
                (unsigned long long)k, (unsigned long long)nelem);
  if ((uintptr_t)payload % 16)
    return fail(BYTEPS_REDUCE_EARGS, "segment %d: payload is not 16-byte aligned", seg);
  return BYTEPS_REDUCE_OK;
}

// The compress's scratch of a plan of p->nsegs segments and p->nrecs tiles.
hipError_t alloc_scratch(byteps_reduce_topk_plan* p) {
  hipError_t e = hipSuccess;
  if (p->nsegs) {
    e = hipMalloc(&p->hist, (size_t)p->nsegs * kTopKBins * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&p->pick, (size_t)p->nsegs * sizeof(TopKPick));
  }
  if (e == hipSuccess && p->nrecs) {
    e = hipMalloc(&p->count, (size_t)p->nrecs * sizeof(TopKCount));
    if (e == hipSuccess) e = hipMalloc(&p->before, (size_t)p->nrecs * sizeof(TopKCount));
  }
  return e;
}

TopKCompress compress_args(const byteps_reduce_topk_plan* p) {
  return TopKCompress{static_cast<const TopKRec*>(p->table),
                      static_cast<const TopKSeg*>(p->side),
                      static_cast<uint32_t*>(p->hist),
                      static_cast<TopKPick*>(p->pick),
                      static_cast<TopKCount*>(p->count),
                      static_cast<TopKCount*>(p->before),
                      p->nrecs,
                      p->nsegs};
}

}  // namespace

}  // namespace bpsr

using namespace bpsr;

extern "C" {

uint64_t byteps_reduce_topk_payload_bytes(uint64_t k) { return topk_payload_bytes(k); }

int byteps_reduce_topk_plan_create(const byteps_topk_desc* segs, int nsegs,
                                   byteps_reduce_topk_plan** out) {
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null plan out-pointer");
  *out = nullptr;
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  std::vector<TopKRec> recs;
  std::vector<TopKSeg> stab((size_t)nsegs);
  std::vector<Range> ranges;
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_topk_desc& d = segs[i];
    if (int rc = check_sizes(d.nelem, d.k, d.payload, i)) return rc;
    if (d.nelem > 0 && (!d.grad || !d.resid || !d.payload))
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    // an empty segment still gets its header where it names a payload
    bool ok = !d.payload || add_range(ranges, d.payload, topk_payload_bytes(d.k), i);
    if (d.nelem > 0)
      ok = ok && add_range(ranges, d.grad, d.nelem * 4, i) &&
           add_range(ranges, d.resid, d.nelem * 4, i);
    if (!ok) return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    const size_t first = recs.size();
    cut(recs, static_cast<unsigned char*>(const_cast<void*>(d.grad)),
        static_cast<unsigned char*>(d.resid), d.nelem, (uint32_t)i);
    stab[(size_t)i] = TopKSeg{static_cast<unsigned char*>(d.payload), d.nelem, (uint32_t)d.k,
                              (uint32_t)first, (uint32_t)(recs.size() - first), 0};
    total += d.nelem;
    if (recs.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_topk_plan();
  p->nrecs = (uint32_t)recs.size();
  p->nsegs = (uint32_t)nsegs;
  p->nelem = total;
  hipError_t e = upload(&p->table, recs);
  if (e == hipSuccess) e = upload(&p->side, stab);
  if (e == hipSuccess) e = alloc_scratch(p);
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "topk plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_topk_plan_compress(byteps_reduce_topk_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (p->fold)
    return fail(BYTEPS_REDUCE_EARGS,
                "compress on a fold plan (byteps_reduce_topk_fold_plan_launch)");
  if (p->refold)
    return fail(BYTEPS_REDUCE_EARGS,
                "compress on a refold plan (byteps_reduce_topk_refold_plan_launch)");
  const TopKCompress a = compress_args(p);
  // more than 4 sources: the process-wide tuning as it stands
  const hipError_t e = launch_topk_compress(a, p->nelem * 4, launch_tuning_for_n(kTopKMaxSrcs),
                                            stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "topk compress kernel launch");
}

int byteps_reduce_topk_fold_plan_create(const byteps_topk_fold_desc* segs, int nsegs, int nsrc,
                                        byteps_reduce_topk_plan** out) {
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null plan out-pointer");
  *out = nullptr;
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  if (nsrc < 1 || nsrc > kTopKMaxSrcs)
    return fail(BYTEPS_REDUCE_EARGS, "nsrc %d outside 1..%d", nsrc, kTopKMaxSrcs);
  std::vector<TopKRec> recs;
  std::vector<TopKSeg> stab((size_t)nsegs);
  std::vector<const unsigned char*> rows((size_t)nsegs * (size_t)nsrc, nullptr);
  std::vector<Range> ranges;
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_topk_fold_desc& d = segs[i];
    if (int rc = check_sizes(d.nelem, d.k, nullptr, i)) return rc;
    stab[(size_t)i] = TopKSeg{nullptr, d.nelem, (uint32_t)d.k, (uint32_t)recs.size(), 0, 0};
    if (d.nelem == 0) continue;
    if (!d.out || !d.payloads) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    bool ok = add_range(ranges, d.out, d.nelem * 4, i);
    for (int s = 0; s < nsrc; ++s) {
      const void* pl = d.payloads[s];
      if (!pl) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null payload %d", i, s);
      if (int rc = check_sizes(d.nelem, d.k, pl, i)) return rc;
      ok = ok && add_range(ranges, pl, topk_payload_bytes(d.k), i);
      rows[(size_t)i * (size_t)nsrc + (size_t)s] = static_cast<const unsigned char*>(pl);
    }
    if (!ok) return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    cut(recs, static_cast<unsigned char*>(d.out), nullptr, d.nelem, (uint32_t)i);
    stab[(size_t)i].nrecs = (uint32_t)(recs.size() - stab[(size_t)i].rec_begin);
    total += d.nelem;
    if (recs.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_topk_plan();
  p->fold = true;
  p->nsrc = nsrc;
  p->nrecs = (uint32_t)recs.size();
  p->nsegs = (uint32_t)nsegs;
  p->nelem = total;
  hipError_t e = upload(&p->table, recs);
  if (e == hipSuccess) e = upload(&p->side, stab);
  if (e == hipSuccess) e = upload(&p->rows, rows);
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "topk fold plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_topk_fold_plan_launch(byteps_reduce_topk_plan* p, int divisor, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (!p->fold) return fail(BYTEPS_REDUCE_EARGS, "fold launch on a compress plan");
  if (divisor < 1) return fail(BYTEPS_REDUCE_EARGS, "divisor %d < 1", divisor);
  const TopKFold a{static_cast<const TopKRec*>(p->table),
                   static_cast<const TopKSeg*>(p->side),
                   static_cast<const unsigned char* const*>(p->rows),
                   p->nrecs,
                   p->nsrc,
                   divisor};
  const hipError_t e = launch_topk_fold(a, p->nelem * 4, launch_tuning_for_n(kTopKMaxSrcs),
                                        stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "topk fold kernel launch");
}

int byteps_reduce_topk_refold_plan_create(const byteps_topk_refold_desc* segs, int nsegs, int nsrc,
                                          byteps_reduce_topk_plan** out) {
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null plan out-pointer");
  *out = nullptr;
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  if (nsrc < 1 || nsrc > kTopKMaxSrcs)
    return fail(BYTEPS_REDUCE_EARGS, "nsrc %d outside 1..%d", nsrc, kTopKMaxSrcs);
  std::vector<TopKRec> recs;
  std::vector<TopKSeg> stab((size_t)nsegs);
  std::vector<const unsigned char*> rows((size_t)nsegs * (size_t)nsrc, nullptr);
  std::vector<Range> ranges;
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_topk_refold_desc& d = segs[i];
    if (int rc = check_sizes(d.nelem, d.k, d.out, i)) return rc;
    if (d.nelem > 0 && (!d.srcs || !d.resid || !d.out))
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    if ((uintptr_t)d.resid % 4)
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: residual is not 4-byte aligned", i);
    // an empty segment still gets its header where it names a payload
    bool ok = !d.out || add_range(ranges, d.out, topk_payload_bytes(d.k), i);
    if (d.nelem > 0) {
      ok = ok && add_range(ranges, d.resid, d.nelem * 4, i);
      for (int s = 0; s < nsrc; ++s) {
        const void* pl = d.srcs[s];
        if (!pl) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null payload %d", i, s);
        if (int rc = check_sizes(d.nelem, d.k, pl, i)) return rc;
        ok = ok && add_range(ranges, pl, topk_payload_bytes(d.k), i);
        rows[(size_t)i * (size_t)nsrc + (size_t)s] = static_cast<const unsigned char*>(pl);
      }
    }
    if (!ok) return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    const size_t first = recs.size();
    // the records name the residual twice: the passes behind the first read b alone
    cut(recs, static_cast<unsigned char*>(d.resid), static_cast<unsigned char*>(d.resid), d.nelem,
        (uint32_t)i);
    stab[(size_t)i] = TopKSeg{static_cast<unsigned char*>(d.out), d.nelem, (uint32_t)d.k,
                              (uint32_t)first, (uint32_t)(recs.size() - first), 0};
    total += d.nelem;
    if (recs.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_topk_plan();
  p->refold = true;
  p->nsrc = nsrc;
  p->nrecs = (uint32_t)recs.size();
  p->nsegs = (uint32_t)nsegs;
  p->nelem = total;
  hipError_t e = upload(&p->table, recs);
  if (e == hipSuccess) e = upload(&p->side, stab);
  if (e == hipSuccess) e = upload(&p->rows, rows);
  if (e == hipSuccess) e = alloc_scratch(p);
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "topk refold plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_topk_refold_plan_launch(byteps_reduce_topk_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (!p->refold) return fail(BYTEPS_REDUCE_EARGS, "refold launch on a plan of another kind");
  const TopKRefold a{compress_args(p), static_cast<const unsigned char* const*>(p->rows), p->nsrc};
  const hipError_t e = launch_topk_refold(a, p->nelem * 4, launch_tuning_for_n(kTopKMaxSrcs),
                                          stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "topk refold kernel launch");
}

int byteps_reduce_topk_plan_destroy(byteps_reduce_topk_plan* p) {
  if (!p) return BYTEPS_REDUCE_OK;
  const hipError_t e = plan_free(p);
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "topk plan free");
}

}  // extern "C"
