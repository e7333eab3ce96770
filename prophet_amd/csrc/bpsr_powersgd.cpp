// PowerSGD low-rank compression with error feedback, host side
// (byteps_reduce_powersgd_*, include/bpsr/reduce.h): the operand checks, the
// plan's tables and scratch (bpsr_powersgd.h) and the C entry points.  Every
// check runs before the first HIP call of its entry: a refused call has
// touched nothing.
#include <algorithm>

#include "bpsr_api_internal.h"
#include "bpsr_powersgd.h"

struct byteps_reduce_powersgd_plan {
  uint32_t nsegs = 0;
  uint32_t nrecs[3] = {0, 0, 0};  // PROJECT-P, PROJECT-Q, FINISH
  uint64_t most_p = 0, most_q = 0;  // the largest n r, m r (REDUCE's grid)
  // on the device: the segments, the three phases' records, the partials
  void* segs = nullptr;
  void* recs[3] = {nullptr, nullptr, nullptr};
  void* scratch = nullptr;
};

namespace bpsr {

namespace {

struct Range {
  uintptr_t begin, end;
  int seg;
  const char* what;
};

// All ranges pairwise disjoint (bpsr_cast_table.cpp's sweep).
int check_disjoint(std::vector<Range>& ranges) {
  std::sort(ranges.begin(), ranges.end(),
            [](const Range& a, const Range& b) { return a.begin < b.begin; });
  for (size_t k = 1, far = 0; k < ranges.size(); ++k) {
    if (ranges[k].begin < ranges[far].end)
      return fail(BYTEPS_REDUCE_EARGS, "%s of segment %d overlaps %s of segment %d",
                  ranges[far].what, ranges[far].seg, ranges[k].what, ranges[k].seg);
    if (ranges[k].end > ranges[far].end) far = k;
  }
  return BYTEPS_REDUCE_OK;
}

template <class T>
hipError_t upload(void** dev, const std::vector<T>& host) {
  if (host.empty()) return hipSuccess;
  const size_t bytes = host.size() * sizeof(T);
  const hipError_t e = hipMalloc(dev, bytes);
  return e == hipSuccess ? hipMemcpy(*dev, host.data(), bytes, hipMemcpyHostToDevice) : e;
}

hipError_t plan_free(byteps_reduce_powersgd_plan* p) {
  hipError_t e = hipSuccess;
  for (void* q : {p->segs, p->recs[0], p->recs[1], p->recs[2], p->scratch})
    if (q) {
      const hipError_t e2 = hipFree(q);
      if (e == hipSuccess) e = e2;
    }
  delete p;
  return e;
}

bool shape_ok(uint64_t n, uint64_t m, int rank) {
  return rank >= 1 && rank <= (int)kPsgdMaxRank && n >= 1 && m >= 1 && n <= kPsgdMaxDim &&
         m <= kPsgdMaxDim && n * m <= kPsgdMaxElems;
}

PsgdArgs args_of(const byteps_reduce_powersgd_plan* p, int phase) {
  return PsgdArgs{static_cast<const PsgdSeg*>(p->segs),
                  phase < 0 ? nullptr : static_cast<const PsgdRec*>(p->recs[phase]),
                  phase < 0 ? 0u : p->nrecs[phase], p->nsegs};
}

}  // namespace

}  // namespace bpsr

using namespace bpsr;

extern "C" {

uint64_t byteps_reduce_powersgd_scratch_bytes(uint64_t n, uint64_t m, int rank) {
  return shape_ok(n, m, rank) ? psgd_scratch_elems(n, m, (uint32_t)rank) * 4 : 0;
}

int byteps_reduce_powersgd_plan_create(const byteps_powersgd_desc* segs, int nsegs, int rank,
                                       byteps_reduce_powersgd_plan** out) {
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null plan out-pointer");
  *out = nullptr;
  if (nsegs < 0 || nsegs > 65535 || (nsegs > 0 && !segs))
    return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  if (rank < 1 || rank > (int)kPsgdMaxRank)
    return fail(BYTEPS_REDUCE_EARGS, "rank %d outside 1..%u", rank, kPsgdMaxRank);
  const uint32_t r = (uint32_t)rank;
  std::vector<PsgdSeg> stab((size_t)nsegs);
  std::vector<uint64_t> scratch_at((size_t)nsegs);
  std::vector<PsgdRec> recs[3];
  std::vector<Range> ranges;
  uint64_t scratch = 0, most_p = 0, most_q = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_powersgd_desc& d = segs[i];
    if (!shape_ok(d.n, d.m, rank))
      return fail(BYTEPS_REDUCE_EARGS,
                  "segment %d: a %llu x %llu matrix (1..2^24 each way, 2^33 elements at most)", i,
                  (unsigned long long)d.n, (unsigned long long)d.m);
    const uint64_t big = d.n * d.m * 4, pb = d.n * r * 4, qb = d.m * r * 4;
    const struct {
      const void* p;
      uint64_t bytes;
      const char* what;
    } ops[] = {{d.grad, big, "g"}, {d.resid, big, "R"}, {d.p, pb, "P"},
               {d.q, qb, "Q"},     {d.qn, qb, "Qn"},    {d.out, big, "out"}};
    for (const auto& o : ops) {
      if (!o.p) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null %s", i, o.what);
      if ((uintptr_t)o.p % 16)
        return fail(BYTEPS_REDUCE_EARGS, "segment %d: %s is not 16-byte aligned", i, o.what);
      if (o.bytes > UINTPTR_MAX - (uintptr_t)o.p)
        return fail(BYTEPS_REDUCE_EARGS, "segment %d: %s wraps the address space", i, o.what);
      // out may BE g (FINISH writes the gradient in place); any other overlap is refused
      if (&o == &ops[5] && d.out == d.grad) continue;
      ranges.push_back({(uintptr_t)o.p, (uintptr_t)o.p + (uintptr_t)o.bytes, i, o.what});
    }
    PsgdSeg& S = stab[(size_t)i];
    S = PsgdSeg{static_cast<const float*>(d.grad), static_cast<float*>(d.resid),
                static_cast<float*>(d.p),          static_cast<const float*>(d.q),
                static_cast<float*>(d.qn),         static_cast<float*>(d.out),
                nullptr,                           (uint32_t)d.n,
                (uint32_t)d.m,                     r,
                psgd_kc(d.n, d.m, r),              0,
                psgd_rc(d.n, d.m, r),              0,
                d.m % 4 == 0 ? 1u : 0u};
    S.pchunks = psgd_ceil(d.m, S.kc);
    S.qchunks = psgd_ceil(d.n, S.rc);
    scratch_at[(size_t)i] = scratch;
    scratch += (psgd_scratch_elems(d.n, d.m, r) + 3) & ~3ull;  // 16-byte aligned partials
    most_p = std::max<uint64_t>(most_p, d.n * r);
    most_q = std::max<uint64_t>(most_q, d.m * r);
    const uint32_t s = (uint32_t)i;
    for (uint32_t a = 0; a < psgd_ceil(d.n, kPsgdPRows); ++a)
      for (uint32_t b = 0; b < S.pchunks; ++b) recs[0].push_back({s, a, b});
    for (uint32_t a = 0; a < psgd_ceil(d.m, kPsgdQCols); ++a)
      for (uint32_t b = 0; b < S.qchunks; ++b) recs[1].push_back({s, a, b});
    for (uint32_t a = 0; a < psgd_ceil(d.n, kPsgdFRows); ++a)
      for (uint32_t b = 0; b < psgd_ceil(d.m, kPsgdFCols); ++b) recs[2].push_back({s, a, b});
    for (const auto& v : recs)
      if (v.size() >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  }
  if (int rc = check_disjoint(ranges)) return rc;
  auto* p = new byteps_reduce_powersgd_plan();
  p->nsegs = (uint32_t)nsegs;
  p->most_p = most_p;
  p->most_q = most_q;
  // the scratch is the plan's own allocation: it overlaps no operand
  hipError_t e = scratch ? hipMalloc(&p->scratch, scratch * 4) : hipSuccess;
  for (int i = 0; i < nsegs; ++i)
    stab[(size_t)i].scratch = static_cast<float*>(p->scratch) + scratch_at[(size_t)i];
  if (e == hipSuccess) e = upload(&p->segs, stab);
  for (int k = 0; k < 3 && e == hipSuccess; ++k) {
    p->nrecs[k] = (uint32_t)recs[k].size();
    e = upload(&p->recs[k], recs[k]);
  }
  if (e != hipSuccess) {
    (void)plan_free(p);
    return hip_fail(e, "powersgd plan upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_powersgd_plan_project_p(byteps_reduce_powersgd_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  hipError_t e = launch_psgd_project_p(args_of(p, 0), stream_of(stream));
  if (e == hipSuccess) e = launch_psgd_reduce(args_of(p, -1), false, p->most_p, stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "powersgd project_p launch");
}

int byteps_reduce_powersgd_plan_orthogonalize(byteps_reduce_powersgd_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  const hipError_t e = launch_psgd_orthogonalize(args_of(p, -1), stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "powersgd orthogonalize launch");
}

int byteps_reduce_powersgd_plan_project_q(byteps_reduce_powersgd_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  hipError_t e = launch_psgd_project_q(args_of(p, 1), stream_of(stream));
  if (e == hipSuccess) e = launch_psgd_reduce(args_of(p, -1), true, p->most_q, stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "powersgd project_q launch");
}

int byteps_reduce_powersgd_plan_finish(byteps_reduce_powersgd_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  const hipError_t e = launch_psgd_finish(args_of(p, 2), stream_of(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "powersgd finish launch");
}

int byteps_reduce_powersgd_plan_destroy(byteps_reduce_powersgd_plan* p) {
  if (!p) return BYTEPS_REDUCE_OK;
  const hipError_t e = plan_free(p);
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "powersgd plan free");
}

}  // extern "C"
