// CPU test of the error-feedback cast plan's table builder (build_cast_table_ef,
// prophet_amd/csrc/bpsr_cast_table.cpp, built unchanged by
// tests/test_cast_table_ef.py, plain and under ASan + UBSan).  Every accepted
// table is walked: each element of each segment is covered exactly once, by a
// vector record only where all three operands co-align (worked out here by
// brute force, not with cast_cut_ef), and every record's residual pointer is
// its segment's residual plus (the record's wide pointer - the segment's
// wide pointer).  With the residuals co-aligned the records are those of the
// plain builder, byte for byte.  Overlap between any two of the 3 * nsegs
// ranges, a null residual and a non-f32 wide dtype are rejected with nothing
// written.  The operands are made-up addresses; nothing is read or written
// through them.
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

// nelem f32 elements; the three operands `*_off` BYTES past a 4-KiB boundary
static byteps_cast_ef_desc seg(size_t nelem, size_t wide_off = 0, size_t half_off = 0,
                               size_t resid_off = 0) {
  byteps_cast_ef_desc d;
  d.wide = take(nelem * 4, wide_off);
  d.half = take(nelem * 2, half_off);
  d.resid = take(nelem * 4, resid_off);
  d.nelem = nelem;
  return d;
}

struct Want {
  bool aligned;
  uint64_t head, nunits;
};
// the first element at which all three operands are 16-byte aligned
static Want want_cut(const byteps_cast_ef_desc& d) {
  const uintptr_t w = (uintptr_t)d.wide, h = (uintptr_t)d.half, r = (uintptr_t)d.resid;
  Want c{w % 4 == 0 && h % 2 == 0 && r % 4 == 0, 0, 0};
  if (!c.aligned) return c;
  for (uint64_t e = 0; e < 8 && e < d.nelem; ++e)
    if ((w + e * 4) % 16 == 0 && (h + e * 2) % 16 == 0 && (r + e * 4) % 16 == 0) {
      if ((d.nelem - e) / 8 > 0) c.head = e, c.nunits = (d.nelem - e) / 8;
      break;
    }
  return c;
}

static CastRec record(const std::vector<char>& out, uint32_t i) {
  CastRec r;
  std::memcpy(&r, out.data() + (size_t)i * sizeof(CastRec), sizeof(r));
  return r;
}

static void accept(const std::string& name, const std::vector<byteps_cast_ef_desc>& segs,
                   int copy_vpt, int want_u, long want_records = -1) {
  g_case = name;
  std::vector<char> out(5, 'x');
  std::vector<unsigned char*> rt(3, nullptr);
  CastTableInfo ti;
  const int rc =
      build_cast_table_ef(segs.data(), (int)segs.size(), kFloat32, copy_vpt, out, rt, &ti);
  CHECK(rc == BYTEPS_REDUCE_OK, "rc %d (%s)", rc, g_msg.c_str());
  if (rc != BYTEPS_REDUCE_OK) return;
  std::vector<size_t> live;
  uint64_t total = 0;
  for (size_t i = 0; i < segs.size(); ++i)
    if (segs[i].nelem) live.push_back(i), total += segs[i].nelem;
  CHECK(ti.u == want_u, "u %d, want %d", ti.u, want_u);
  CHECK(ti.live == (int)live.size(), "live %d", ti.live);
  CHECK(ti.nelem == total, "nelem %llu", (unsigned long long)ti.nelem);
  CHECK(out.size() == (size_t)ti.records * sizeof(CastRec), "out %zu records %u", out.size(),
        ti.records);
  CHECK(rt.size() == (size_t)ti.records, "residual pointers %zu, records %u", rt.size(),
        ti.records);
  if (want_records >= 0)
    CHECK(ti.records == (uint32_t)want_records, "records %u, want %ld", ti.records, want_records);
  if (out.size() != (size_t)ti.records * sizeof(CastRec) || rt.size() != ti.records) return;
  const uint64_t tile_units = (uint64_t)kBlock * (uint64_t)ti.u;
  std::vector<std::vector<unsigned char>> cover(live.size());
  for (size_t j = 0; j < live.size(); ++j) cover[j].assign(segs[live[j]].nelem, 0);
  bool full_seen = false;
  for (uint32_t i = 0; i < ti.records; ++i) {
    const CastRec r = record(out, i);
    const uintptr_t w = (uintptr_t)r.wide;
    size_t j = live.size();
    for (size_t k = 0; k < live.size(); ++k) {
      const byteps_cast_ef_desc& d = segs[live[k]];
      if (w >= (uintptr_t)d.wide && w < (uintptr_t)d.wide + d.nelem * 4) j = k;
    }
    CHECK(j < live.size(), "record %u: wide pointer in no segment", i);
    if (j == live.size()) return;
    const byteps_cast_ef_desc& d = segs[live[j]];
    const Want c = want_cut(d);
    const uint64_t off = w - (uintptr_t)d.wide;
    // the residual pointer: segment residual + (rec.wide - segment wide)
    CHECK((uintptr_t)rt[i] == (uintptr_t)d.resid + off, "record %u: residual pointer %p", i,
          (void*)rt[i]);
    CHECK(off % 4 == 0, "record %u: wide offset %llu", i, (unsigned long long)off);
    const uint64_t first = off / 4;
    CHECK((uintptr_t)r.half == (uintptr_t)d.half + first * 2, "record %u: half pointer", i);
    uint64_t n = 0;
    unsigned char mark = 0;
    if (r.kind == kTileElem) {
      CHECK(!full_seen, "record %u: element record after a full tile", i);
      CHECK(r.count >= 1 && r.count <= kCastElemPart, "record %u: count %u", i, r.count);
      CHECK(r.aligned == (uint32_t)c.aligned, "record %u: aligned %u", i, r.aligned);
      n = r.count, mark = 1;
    } else if (r.kind == kTilePartial) {
      CHECK(!full_seen, "record %u: partial tile after a full tile", i);
      CHECK(r.count >= 1 && r.count < tile_units, "record %u: count %u", i, r.count);
      n = 8ull * r.count, mark = 2;
    } else {
      CHECK(r.kind == kTileFull, "record %u: kind %u", i, r.kind);
      CHECK(r.count == tile_units, "record %u: count %u", i, r.count);
      full_seen = true;
      n = 8ull * tile_units, mark = 2;
    }
    if (mark == 2) {
      CHECK(w % 16 == 0 && (uintptr_t)r.half % 16 == 0 && (uintptr_t)rt[i] % 16 == 0,
            "record %u: vector record not 16-byte aligned on all three operands", i);
      CHECK(c.nunits > 0 && first >= c.head && first + n <= c.head + 8 * c.nunits,
            "record %u: vector record outside the vector range", i);
    }
    CHECK(first + n <= d.nelem, "record %u: reaches past its segment", i);
    if (first + n > d.nelem) return;
    for (uint64_t e = first; e < first + n; ++e) {
      CHECK(cover[j][e] == 0, "record %u: element %llu covered twice", i, (unsigned long long)e);
      cover[j][e] = mark;
    }
  }
  for (size_t j = 0; j < live.size(); ++j) {
    const byteps_cast_ef_desc& d = segs[live[j]];
    const Want c = want_cut(d);
    for (uint64_t e = 0; e < d.nelem; ++e) {
      const bool vec = c.nunits && e >= c.head && e < c.head + 8 * c.nunits;
      if (cover[j][e] != (vec ? 2 : 1)) {
        CHECK(false, "segment %zu element %llu: covered by %d, want %d", live[j],
              (unsigned long long)e, cover[j][e], vec ? 2 : 1);
        break;
      }
    }
  }
}

static void reject(const std::string& name, const std::vector<byteps_cast_ef_desc>& segs,
                   int dtype, int want_rc) {
  g_case = name;
  std::vector<char> out(5, 'x');
  std::vector<unsigned char*> rt(3, nullptr);
  CastTableInfo ti;
  g_msg.clear();
  const int rc = build_cast_table_ef(segs.data(), (int)segs.size(), dtype, 2, out, rt, &ti);
  CHECK(rc == want_rc, "rc %d, want %d (%s)", rc, want_rc, g_msg.c_str());
  CHECK(out == std::vector<char>(5, 'x') && rt == std::vector<unsigned char*>(3, nullptr),
        "outputs written on an error");
  CHECK(!g_msg.empty(), "no error text");
}

// With co-aligned residuals the records are the plain builder's, byte for byte.
static void same_records_as_plain() {
  g_case = "same records as the plain table";
  std::vector<byteps_cast_ef_desc> ef = {seg(5000, 4, 2, 4), seg(9), seg(2048 * 3 + 13, 0, 0, 0),
                                         seg(1, 8, 0, 8)};
  std::vector<byteps_cast_desc> plain;
  for (const auto& d : ef) plain.push_back({d.wide, d.half, d.nelem});
  std::vector<char> a, b;
  std::vector<unsigned char*> rt;
  CastTableInfo ta, tb;
  const int ra = build_cast_table_ef(ef.data(), (int)ef.size(), kFloat32, 2, a, rt, &ta);
  const int rb = build_cast_table(plain.data(), (int)plain.size(), kFloat32, 2, b, &tb);
  CHECK(ra == BYTEPS_REDUCE_OK && rb == BYTEPS_REDUCE_OK, "rc %d %d", ra, rb);
  CHECK(a == b && ta.records == tb.records && ta.u == tb.u, "tables differ");
}

int main() {
  // sizes around one unit and one tile, the three operands co-aligned
  for (size_t n : {1, 7, 8, 9, 2047, 2048, 2049, 2056, 3 * 2048 + 13})
    accept("aligned n=" + std::to_string(n), {seg(n)}, 2, 1);
  // wide and residual 0..3 elements past a boundary, independently; the wire
  // side co-aligning with the wide one (2 bytes an element) or not
  for (size_t w = 0; w < 4; ++w)
    for (size_t r = 0; r < 4; ++r)
      for (size_t h : {(size_t)0, w * 2, (size_t)2, (size_t)14})
        accept("offsets w=" + std::to_string(w) + " r=" + std::to_string(r) + " h=" +
                   std::to_string(h),
               {seg(2048 + 77, w * 4, h, r * 4)}, 2, 1);
  // element-misaligned operands: everything through the element path, aligned = 0
  accept("wide byte-misaligned", {seg(300, 1, 0, 0)}, 2, 1, 1);
  accept("residual byte-misaligned", {seg(300, 0, 0, 2)}, 2, 1, 1);
  accept("wire byte-misaligned", {seg(300, 0, 1, 0)}, 2, 1, 1);
  // a long segment whose residual never co-aligns is split into element parts
  accept("never co-aligned, split", {seg(3 * kCastElemPart + 5, 0, 0, 4)}, 2, 1, 4);
  // a mixed plan: empty, 1 element, never co-aligned, partial tile, one and several tiles
  accept("mixed", {seg(0), seg(1), seg(500, 0, 0, 8), seg(1000), seg(2048), seg(5 * 2048, 4, 2, 4)},
         2, 1);
  // enough tiles for two and for four units a lane
  accept("u=2", {seg((size_t)kMinTiles * 2 * 2048 + 11, 4, 2, 4)}, 2, 2);
  accept("u=4", {seg((size_t)kMinTiles * 4 * 2048 + 11)}, 4, 4);
  accept("empty plan", {}, 2, 1, 0);
  accept("only empty segments", {seg(0), seg(0)}, 2, 1, 0);
  same_records_as_plain();

  // overlap between any two of the 3 * nsegs ranges
  {
    byteps_cast_ef_desc a = seg(100), b = seg(100);
    const char* names[3] = {"wide", "half", "resid"};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        // b's operand j starts inside a's operand i
        byteps_cast_ef_desc x = b;
        void* const src[3] = {a.wide, a.half, a.resid};
        void** dst[3] = {&x.wide, &x.half, &x.resid};
        *dst[j] = static_cast<char*>(src[i]) + 4;
        reject(std::string("overlap a.") + names[i] + " / b." + names[j], {a, x}, kFloat32,
               BYTEPS_REDUCE_EARGS);
      }
    // within one segment
    byteps_cast_ef_desc s = seg(100);
    byteps_cast_ef_desc t = s;
    t.resid = s.wide;
    reject("resid == wide", {t}, kFloat32, BYTEPS_REDUCE_EARGS);
    t = s;
    t.resid = static_cast<char*>(s.half) + 198;
    reject("resid on the wire side's last bytes", {t}, kFloat32, BYTEPS_REDUCE_EARGS);
    t = s;
    t.half = static_cast<char*>(s.resid) + 396;
    reject("wire on the residual's last bytes", {t}, kFloat32, BYTEPS_REDUCE_EARGS);
    // touching ranges are fine
    t = s;
    t.resid = static_cast<char*>(s.wide) + 400;
    t.half = static_cast<char*>(s.wide) + 800;
    accept("touching ranges", {t}, 2, 1);
  }
  {
    byteps_cast_ef_desc s = seg(16);
    byteps_cast_ef_desc t = s;
    t.resid = nullptr;
    reject("null residual", {t}, kFloat32, BYTEPS_REDUCE_EARGS);
    t = s;
    t.wide = nullptr;
    reject("null wide", {t}, kFloat32, BYTEPS_REDUCE_EARGS);
    t.nelem = 0;  // an empty segment may carry null pointers
    t.resid = nullptr;
    accept("null pointers, nelem 0", {t}, 2, 1, 0);
    for (int dt : {(int)kFloat64, (int)kBFloat16, (int)kFloat16, 4, 99})
      reject("dtype " + std::to_string(dt), {s}, dt, BYTEPS_REDUCE_EDTYPE);
    g_case = "bad table";
    std::vector<char> out;
    std::vector<unsigned char*> rt;
    CastTableInfo ti;
    CHECK(build_cast_table_ef(nullptr, 1, kFloat32, 2, out, rt, &ti) == BYTEPS_REDUCE_EARGS,
          "null table");
    CHECK(build_cast_table_ef(&s, -1, kFloat32, 2, out, rt, &ti) == BYTEPS_REDUCE_EARGS,
          "negative count");
  }
  printf("fails=%d\n", g_fails);
  return g_fails ? 1 : 0;
}
