// CPU test of the segment record lists the cast table builders make for the
// decompress statistics (CastSegList; build_cast_table / _ef / _sr with a
// `lists` argument, prophet_amd/csrc/bpsr_cast_table.cpp, built unchanged by
// tests/test_cast_table_stats.py, plain and under ASan + UBSan).  Every record
// appears once, under the segment whose wide range contains it; within a
// segment the records ascend; empty segments have empty lists; the CastRec
// bytes (and an EF plan's residual pointers, an SR plan's parallel entries)
// equal those of the builder without lists; on an error nothing is written.
// The operands are made-up addresses; nothing is read or written through them.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bpsr_api_internal.h"

namespace bpsr {
// stand-ins for bpsr_api.cpp (HIP): the error text and the default tuning
static std::string g_msg;
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_msg = buf;
  return code;
}
Tuning launch_tuning_for_n(int) {
  return Tuning{2, 1, 1 << 20, 1, 2, 0, 4096, 4096, 1, 4, 2, kWtMaxBytes};
}
}  // namespace bpsr

using namespace bpsr;

static int g_fails = 0;
static std::string g_case;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    if (!(cond)) {                                                        \
      if (++g_fails <= 40) {                                              \
        printf("FAIL %s line %d: %s: ", g_case.c_str(), __LINE__, #cond); \
        printf(__VA_ARGS__);                                              \
        printf("\n");                                                     \
      }                                                                   \
    }                                                                     \
  } while (0)

static uintptr_t g_next = (uintptr_t)1 << 32;
static void* take(size_t bytes, size_t off) {
  g_next = (g_next + 4095) & ~(uintptr_t)4095;
  const uintptr_t p = g_next + off;
  g_next = p + bytes + 256;
  return reinterpret_cast<void*>(p);
}

// One segment of every kind of plan: `es` bytes a wide element, the operands
// `*_off` BYTES past a 4-KiB boundary, the residual co-aligned with the wide
// operand.
struct Seg {
  void *wide, *half, *resid;
  size_t nelem;
  uint32_t key;
};
static Seg seg(size_t nelem, int es = 4, size_t wide_off = 0, size_t half_off = 0) {
  Seg s;
  s.wide = take(nelem * (size_t)es, wide_off);
  s.half = take(nelem * 2, half_off);
  s.resid = take(nelem * 4, wide_off);
  s.nelem = nelem;
  s.key = (uint32_t)(nelem * 2654435761u + 1);
  return s;
}

static CastRec record(const std::vector<char>& out, uint32_t i) {
  CastRec r;
  std::memcpy(&r, out.data() + (size_t)i * sizeof(CastRec), sizeof(r));
  return r;
}

enum Kind { kPlain, kEf, kSr };
static const char* kNames[] = {"plain", "ef", "sr"};

// Runs builder `kind` with (lists != null) or without the lists.
static int run(Kind kind, const std::vector<Seg>& segs, int dtype, int copy_vpt,
               std::vector<char>& out, std::vector<unsigned char*>& rt, std::vector<CastSrRec>& st,
               CastTableInfo* ti, CastSegList* lists, bool with_lists) {
  const int n = (int)segs.size();
  if (kind == kPlain) {
    std::vector<byteps_cast_desc> d;
    for (const Seg& s : segs) d.push_back({s.wide, s.half, s.nelem});
    return with_lists ? build_cast_table(d.data(), n, dtype, copy_vpt, out, ti, lists)
                      : build_cast_table(d.data(), n, dtype, copy_vpt, out, ti);
  }
  if (kind == kEf) {
    std::vector<byteps_cast_ef_desc> d;
    for (const Seg& s : segs) d.push_back({s.wide, s.half, s.resid, s.nelem});
    return with_lists ? build_cast_table_ef(d.data(), n, dtype, copy_vpt, out, rt, ti, lists)
                      : build_cast_table_ef(d.data(), n, dtype, copy_vpt, out, rt, ti);
  }
  std::vector<byteps_cast_sr_desc> d;
  for (const Seg& s : segs) {
    byteps_cast_sr_desc x;
    std::memset(&x, 0, sizeof(x));
    x.wide = s.wide;
    x.half = s.half;
    x.nelem = s.nelem;
    x.key = s.key;
    d.push_back(x);
  }
  return with_lists ? build_cast_table_sr(d.data(), n, dtype, copy_vpt, out, st, ti, lists)
                    : build_cast_table_sr(d.data(), n, dtype, copy_vpt, out, st, ti);
}

static void accept(const std::string& name, Kind kind, const std::vector<Seg>& segs, int dtype,
                   int copy_vpt, int want_u) {
  g_case = name + " [" + kNames[kind] + "]";
  const uint64_t es = dtype == kFloat64 ? 8 : dtype == kFloat32 ? 4 : 2;
  std::vector<char> out(5, 'x'), ref;
  std::vector<unsigned char*> rt, rt_ref;
  std::vector<CastSrRec> st, st_ref;
  CastTableInfo ti, tr;
  CastSegList l;
  l.seg_begin.assign(3, 77);
  l.seg_recs.assign(2, 77);
  const int rc = run(kind, segs, dtype, copy_vpt, out, rt, st, &ti, &l, true);
  CHECK(rc == BYTEPS_REDUCE_OK, "rc %d (%s)", rc, g_msg.c_str());
  if (rc != BYTEPS_REDUCE_OK) return;
  const int rr = run(kind, segs, dtype, copy_vpt, ref, rt_ref, st_ref, &tr, nullptr, false);
  CHECK(rr == BYTEPS_REDUCE_OK, "reference rc %d (%s)", rr, g_msg.c_str());
  CHECK(out == ref, "CastRec bytes differ from the builder without lists");
  CHECK(rt == rt_ref, "residual pointers differ");
  CHECK(st.size() == st_ref.size() &&
            (st.empty() || !std::memcmp(st.data(), st_ref.data(), st.size() * sizeof(CastSrRec))),
        "stochastic-rounding entries differ");
  CHECK(ti.u == tr.u && ti.records == tr.records && ti.nelem == tr.nelem && ti.live == tr.live &&
            ti.bytes == tr.bytes,
        "table info differs");
  CHECK(ti.u == want_u, "u %d, want %d", ti.u, want_u);
  // a null `lists` through the new entry point is the old call
  {
    std::vector<char> o2;
    std::vector<unsigned char*> r2;
    std::vector<CastSrRec> s2;
    CastTableInfo t2;
    CHECK(run(kind, segs, dtype, copy_vpt, o2, r2, s2, &t2, nullptr, true) == BYTEPS_REDUCE_OK &&
              o2 == ref,
          "null lists");
  }
  const size_t nsegs = segs.size();
  CHECK(l.seg_begin.size() == nsegs + 1, "seg_begin has %zu entries, want %zu",
        l.seg_begin.size(), nsegs + 1);
  CHECK(l.seg_recs.size() == (size_t)ti.records, "seg_recs has %zu entries, records %u",
        l.seg_recs.size(), ti.records);
  if (l.seg_begin.size() != nsegs + 1 || l.seg_recs.size() != ti.records) return;
  CHECK(l.seg_begin[0] == 0 && l.seg_begin[nsegs] == ti.records, "seg_begin ends %u .. %u",
        l.seg_begin[0], l.seg_begin[nsegs]);
  std::vector<int> seen(ti.records, 0);
  for (size_t j = 0; j < nsegs; ++j) {
    const uint32_t b = l.seg_begin[j], e = l.seg_begin[j + 1];
    CHECK(b <= e && e <= ti.records, "segment %zu: list [%u, %u)", j, b, e);
    if (b > e || e > ti.records) return;
    if (segs[j].nelem == 0) CHECK(b == e, "empty segment %zu owns %u records", j, e - b);
    uint64_t covered = 0;
    for (uint32_t k = b; k < e; ++k) {
      const uint32_t r = l.seg_recs[k];
      CHECK(r < ti.records, "segment %zu: record %u out of range", j, r);
      if (r >= ti.records) return;
      CHECK(k == b || l.seg_recs[k - 1] < r, "segment %zu: records not ascending at %u", j, k);
      ++seen[r];
      const CastRec c = record(out, r);
      CHECK(c.pad == 0, "record %u: pad %u", r, c.pad);
      const uintptr_t w = (uintptr_t)c.wide, w0 = (uintptr_t)segs[j].wide;
      CHECK(w >= w0 && w < w0 + segs[j].nelem * es,
            "record %u listed under segment %zu, whose wide range does not contain it", r, j);
      covered += c.kind == kTileElem ? c.count : 8ull * c.count;
    }
    CHECK(covered == segs[j].nelem, "segment %zu: its records cover %llu of %zu elements", j,
          (unsigned long long)covered, segs[j].nelem);
  }
  for (uint32_t r = 0; r < ti.records; ++r)
    CHECK(seen[r] == 1, "record %u appears %d times", r, seen[r]);
}

static void reject(const std::string& name, Kind kind, const std::vector<Seg>& segs, int dtype,
                   int want_rc) {
  g_case = name + " [" + kNames[kind] + "]";
  std::vector<char> out(5, 'x');
  std::vector<unsigned char*> rt(2, nullptr);
  std::vector<CastSrRec> st(3, CastSrRec{7, 7, 7});
  CastTableInfo ti;
  CastSegList l;
  l.seg_begin.assign(3, 77);
  l.seg_recs.assign(2, 78);
  g_msg.clear();
  const int rc = run(kind, segs, dtype, 2, out, rt, st, &ti, &l, true);
  CHECK(rc == want_rc, "rc %d, want %d (%s)", rc, want_rc, g_msg.c_str());
  CHECK(out == std::vector<char>(5, 'x') && rt.size() == 2 && st.size() == 3,
        "tables written on an error");
  CHECK(l.seg_begin == std::vector<uint32_t>(3, 77) && l.seg_recs == std::vector<uint32_t>(2, 78),
        "lists written on an error");
  CHECK(!g_msg.empty(), "no error text");
}

int main() {
  for (Kind kind : {kPlain, kEf, kSr}) {
    for (size_t n : {1, 7, 8, 9, 2047, 2048, 2049, 2048 + 3 * 8 + 5, 3 * 2048 + 13})
      accept("aligned n=" + std::to_string(n), kind, {seg(n)}, kFloat32, 2, 1);
    accept("head and tail", kind, {seg(2 * 2048 + 77, 4, 4, 2)}, kFloat32, 2, 1);
    accept("never co-aligned, three element records", kind, {seg(2 * kCastElemPart + 5, 4, 0, 2)},
           kFloat32, 2, 1);
    // the records of one segment are NOT contiguous in the table (guarded
    // tiles and element ranges of every segment come first, full tiles last)
    accept("mixed, empty in the middle", kind,
           {seg(5 * 2048 + 3, 4, 4, 2), seg(1), seg(0), seg(2 * 2048), seg(500, 4, 0, 2),
            seg(0), seg(3 * 2048 + 9, 4, 8, 4)},
           kFloat32, 2, 1);
    accept("u=2", kind, {seg(100), seg((size_t)kMinTiles * 2 * 2048 + 11, 4, 4, 2), seg(0)},
           kFloat32, 2, 2);
    accept("u=4", kind, {seg((size_t)kMinTiles * 4 * 2048 + 11), seg(3000)}, kFloat32, 4, 4);
    accept("empty plan", kind, {}, kFloat32, 2, 1);
    accept("only empty segments", kind, {seg(0), seg(0)}, kFloat32, 2, 1);
    // errors: overlap, null pointer, wrong dtype
    {
      Seg a = seg(100), b = seg(100);
      Seg x = b;
      x.wide = static_cast<char*>(a.wide) + 4;
      reject("overlap", kind, {a, x}, kFloat32, BYTEPS_REDUCE_EARGS);
      x = a;
      x.half = nullptr;
      reject("null half", kind, {b, x}, kFloat32, BYTEPS_REDUCE_EARGS);
      reject("dtype 4", kind, {a}, 4, BYTEPS_REDUCE_EDTYPE);
    }
  }
  // the plain builder's other wide dtypes
  accept("f64", kPlain, {seg(2048 + 9, 8), seg(0, 8), seg(700, 8, 8, 2)}, kFloat64, 2, 1);
  accept("2-byte wide", kPlain, {seg(4096 + 9, 2), seg(0, 2), seg(700, 2, 2, 2)}, kBFloat16, 2, 1);
  printf("fails=%d\n", g_fails);
  return g_fails ? 1 : 0;
}
