// CPU test of the stochastic-rounding cast plan's table builder
// (build_cast_table_sr, prophet_amd/csrc/bpsr_cast_table.cpp, built unchanged
// by tests/test_cast_table_sr.py, plain and under ASan + UBSan).  The records
// are the plain builder's byte for byte — the cut is cast_cut, a key changes
// no record — and the parallel array holds, per record, the index in its
// segment of the record's first element (64-bit: a segment of 2^34 elements
// is accepted, one more is not) and the segment's key.  Overlap between any
// two of the 2 * nsegs ranges, a null pointer, a segment that is too long and
// a non-f32 wide dtype are rejected with nothing written.  The operands are
// made-up addresses; nothing is read or written through them.
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

// nelem f32 elements; the two operands `*_off` BYTES past a 4-KiB boundary
static byteps_cast_sr_desc seg(size_t nelem, uint32_t key, size_t wide_off = 0,
                               size_t half_off = 0) {
  byteps_cast_sr_desc d;
  std::memset(&d, 0, sizeof(d));
  d.wide = take(nelem * 4, wide_off);
  d.half = take(nelem * 2, half_off);
  d.nelem = nelem;
  d.key = key;
  return d;
}

static CastRec record(const std::vector<char>& out, uint32_t i) {
  CastRec r;
  std::memcpy(&r, out.data() + (size_t)i * sizeof(CastRec), sizeof(r));
  return r;
}

// Builds the SR table and the plain one over the same operands: equal records,
// and every parallel entry names its record's first element and segment key.
// `cover`: also mark every element (short plans only).
static void accept(const std::string& name, const std::vector<byteps_cast_sr_desc>& segs,
                   int copy_vpt, int want_u, long want_records = -1, bool cover = true) {
  g_case = name;
  std::vector<char> out(5, 'x'), plain_out;
  std::vector<CastSrRec> st(3);
  CastTableInfo ti, tp;
  const int rc =
      build_cast_table_sr(segs.data(), (int)segs.size(), kFloat32, copy_vpt, out, st, &ti);
  CHECK(rc == BYTEPS_REDUCE_OK, "rc %d (%s)", rc, g_msg.c_str());
  if (rc != BYTEPS_REDUCE_OK) return;
  std::vector<byteps_cast_desc> plain;
  for (const auto& d : segs) plain.push_back({d.wide, d.half, d.nelem});
  const int rp =
      build_cast_table(plain.data(), (int)plain.size(), kFloat32, copy_vpt, plain_out, &tp);
  CHECK(rp == BYTEPS_REDUCE_OK, "plain rc %d (%s)", rp, g_msg.c_str());
  CHECK(out == plain_out, "records differ from the plain builder's");
  CHECK(ti.u == tp.u && ti.records == tp.records && ti.nelem == tp.nelem && ti.live == tp.live &&
            ti.bytes == tp.bytes,
        "table info differs from the plain builder's");
  CHECK(ti.u == want_u, "u %d, want %d", ti.u, want_u);
  CHECK(st.size() == (size_t)ti.records, "parallel entries %zu, records %u", st.size(),
        ti.records);
  if (want_records >= 0)
    CHECK(ti.records == (uint32_t)want_records, "records %u, want %ld", ti.records, want_records);
  if (out.size() != (size_t)ti.records * sizeof(CastRec) || st.size() != ti.records) return;
  const uint64_t tile_units = (uint64_t)kBlock * (uint64_t)ti.u;
  std::vector<std::vector<unsigned char>> seen(segs.size());
  if (cover)
    for (size_t j = 0; j < segs.size(); ++j) seen[j].assign(segs[j].nelem, 0);
  for (uint32_t i = 0; i < ti.records; ++i) {
    const CastRec r = record(out, i);
    const uintptr_t w = (uintptr_t)r.wide;
    size_t j = segs.size();
    for (size_t k = 0; k < segs.size(); ++k)
      if (segs[k].nelem && w >= (uintptr_t)segs[k].wide &&
          w < (uintptr_t)segs[k].wide + segs[k].nelem * 4)
        j = k;
    CHECK(j < segs.size(), "record %u: wide pointer in no segment", i);
    if (j == segs.size()) return;
    const byteps_cast_sr_desc& d = segs[j];
    const uint64_t first = (w - (uintptr_t)d.wide) / 4;
    CHECK(st[i].first == first, "record %u: first %llu, want %llu", i,
          (unsigned long long)st[i].first, (unsigned long long)first);
    CHECK(st[i].key == d.key, "record %u: key %x, want %x", i, st[i].key, d.key);
    CHECK(st[i].pad == 0, "record %u: pad %u", i, st[i].pad);
    CHECK((uintptr_t)r.half == (uintptr_t)d.half + first * 2, "record %u: half pointer", i);
    const uint64_t n = r.kind == kTileElem ? r.count : 8ull * r.count;
    if (r.kind == kTileFull) {
      CHECK(r.count == tile_units, "record %u: count %u", i, r.count);
      CHECK(w % 16 == 0 && (uintptr_t)r.half % 16 == 0, "record %u: alignment", i);
    }
    CHECK(first + n <= d.nelem, "record %u: reaches past its segment", i);
    if (!cover || first + n > d.nelem) continue;
    for (uint64_t e = first; e < first + n; ++e) {
      CHECK(seen[j][e] == 0, "record %u: element %llu covered twice", i, (unsigned long long)e);
      seen[j][e] = 1;
    }
  }
  if (cover)
    for (size_t j = 0; j < segs.size(); ++j)
      for (uint64_t e = 0; e < segs[j].nelem; ++e)
        if (!seen[j][e]) {
          CHECK(false, "segment %zu element %llu not covered", j, (unsigned long long)e);
          break;
        }
}

static void reject(const std::string& name, const std::vector<byteps_cast_sr_desc>& segs,
                   int dtype, int want_rc) {
  g_case = name;
  std::vector<char> out(5, 'x');
  std::vector<CastSrRec> st(3, CastSrRec{7, 7, 7});
  CastTableInfo ti;
  g_msg.clear();
  const int rc = build_cast_table_sr(segs.data(), (int)segs.size(), dtype, 2, out, st, &ti);
  CHECK(rc == want_rc, "rc %d, want %d (%s)", rc, want_rc, g_msg.c_str());
  bool same = out == std::vector<char>(5, 'x') && st.size() == 3;
  for (size_t i = 0; same && i < 3; ++i) same = st[i].first == 7 && st[i].key == 7;
  CHECK(same, "outputs written on an error");
  CHECK(!g_msg.empty(), "no error text");
}

int main() {
  // sizes around one unit and one tile
  for (size_t n : {1, 3, 4, 5, 7, 8, 9, 2047, 2048, 2049, 2057, 3 * 2048 + 13})
    accept("aligned n=" + std::to_string(n), {seg(n, 0x1234)}, 2, 1);
  // the wide base 0..3 elements past a 16-byte boundary with the wire side
  // co-aligning after a head (first element index of the tiles = head, 4 - w
  // elements: not a multiple of 4 but for w = 0) or never
  for (size_t w = 0; w < 4; ++w)
    for (size_t h : {(size_t)0, w * 2, (size_t)2, (size_t)14})
      accept("offsets w=" + std::to_string(w) + " h=" + std::to_string(h),
             {seg(2 * 2048 + 77, 0xabcdef01u + (uint32_t)w, w * 4, h)}, 2, 1);
  {
    // wide base one element past a 16-byte boundary (3 elements to the next),
    // wire base one element past (7 to the next): they meet at element 7, so
    // every vector holds elements 4q + 3 .. 4q + 6 and straddles two groups
    g_case = "head of 7";
    std::vector<byteps_cast_sr_desc> s = {seg(2048 + 16, 9, 4, 2)};
    std::vector<char> out;
    std::vector<CastSrRec> st;
    CastTableInfo ti;
    CHECK(build_cast_table_sr(s.data(), 1, kFloat32, 2, out, st, &ti) == BYTEPS_REDUCE_OK, "rc");
    bool full = false;
    for (uint32_t i = 0; i < ti.records; ++i)
      if (record(out, i).kind == kTileFull) {
        full = true;
        CHECK(st[i].first == 7, "first %llu", (unsigned long long)st[i].first);
      }
    CHECK(full, "no full tile");
  }
  accept("wide byte-misaligned", {seg(300, 1, 1, 0)}, 2, 1, 1);
  accept("wire byte-misaligned", {seg(300, 2, 0, 1)}, 2, 1, 1);
  accept("never co-aligned, split", {seg(3 * kCastElemPart + 5, 3, 0, 2)}, 2, 1, 4);
  accept("mixed, distinct keys",
         {seg(0, 1), seg(1, 2), seg(500, 3, 0, 2), seg(1000, 4), seg(2048, 0xffffffffu),
          seg(5 * 2048, 0, 4, 2), seg(2047, 7, 8, 4), seg(2049, 8, 12, 6)},
         2, 1);
  accept("u=2", {seg((size_t)kMinTiles * 2 * 2048 + 11, 5, 4, 2)}, 2, 2);
  accept("u=4", {seg((size_t)kMinTiles * 4 * 2048 + 11, 6)}, 4, 4);
  accept("empty plan", {}, 2, 1, 0);
  accept("only empty segments", {seg(0, 1), seg(0, 2)}, 2, 1, 0);
  // the longest segment: 2^34 elements, its last tile's first index past 2^32
  {
    const size_t big = (size_t)1 << 34;
    std::vector<byteps_cast_sr_desc> s = {seg(big, 0x51, 4, 2), seg(100, 0x52)};
    accept("2^34 elements", s, 4, 4, -1, false);
    g_case = "2^34 elements, last tile";
    std::vector<char> out;
    std::vector<CastSrRec> st;
    CastTableInfo ti;
    CHECK(build_cast_table_sr(s.data(), 2, kFloat32, 4, out, st, &ti) == BYTEPS_REDUCE_OK, "rc");
    uint64_t top = 0;
    for (const CastSrRec& r : st)
      if (r.key == 0x51 && r.first > top) top = r.first;
    CHECK(top > (1ull << 33) && top < big && top % 4 == 3, "largest first index %llu",
          (unsigned long long)top);
    s[0].nelem = big + 1;
    reject("2^34 + 1 elements", s, kFloat32, BYTEPS_REDUCE_EARGS);
  }
  // overlap between any two of the 2 * nsegs ranges
  {
    byteps_cast_sr_desc a = seg(100, 1), b = seg(100, 2);
    const char* names[2] = {"wide", "half"};
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j) {
        byteps_cast_sr_desc x = b;
        void* const src[2] = {a.wide, a.half};
        void** dst[2] = {&x.wide, &x.half};
        *dst[j] = static_cast<char*>(src[i]) + 4;
        reject(std::string("overlap a.") + names[i] + " / b." + names[j], {a, x}, kFloat32,
               BYTEPS_REDUCE_EARGS);
      }
    byteps_cast_sr_desc t = a;
    t.half = static_cast<char*>(a.wide) + 396;
    reject("wire on the wide side's last bytes", {t}, kFloat32, BYTEPS_REDUCE_EARGS);
    t.half = static_cast<char*>(a.wide) + 400;
    accept("touching ranges", {t}, 2, 1);
    t = a;
    t.wide = nullptr;
    reject("null wide", {t}, kFloat32, BYTEPS_REDUCE_EARGS);
    t = a;
    t.half = nullptr;
    reject("null half", {t}, kFloat32, BYTEPS_REDUCE_EARGS);
    t.nelem = 0;  // an empty segment may carry null pointers
    accept("null pointers, nelem 0", {t}, 2, 1, 0);
    for (int dt : {(int)kFloat64, (int)kBFloat16, (int)kFloat16, 4, 99})
      reject("dtype " + std::to_string(dt), {a}, dt, BYTEPS_REDUCE_EDTYPE);
    g_case = "bad table";
    std::vector<char> out;
    std::vector<CastSrRec> st;
    CastTableInfo ti;
    CHECK(build_cast_table_sr(nullptr, 1, kFloat32, 2, out, st, &ti) == BYTEPS_REDUCE_EARGS,
          "null table");
    CHECK(build_cast_table_sr(&a, -1, kFloat32, 2, out, st, &ti) == BYTEPS_REDUCE_EARGS,
          "negative count");
  }
  printf("fails=%d\n", g_fails);
  return g_fails ? 1 : 0;
}
