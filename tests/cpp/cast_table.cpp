// CPU test of the cast plan's table builder (prophet_amd/csrc/bpsr_cast_table.cpp,
// built unchanged by tests/test_cast_table.py, plain and under ASan + UBSan).
// Every table it accepts is walked record by record: each element of each
// segment is covered exactly once, by the kind of record the single cast's cut
// sends it to (worked out here by brute force, not with cast_cut), no record
// reaches outside its segment, the record count is the grid, and the guarded
// and element records come before the full tiles.  The operands are made-up
// addresses; nothing is read or written through them.
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

// Made-up addresses: each operand starts `off` bytes past a 4-KiB boundary
// and is followed by a gap.
static uintptr_t g_next = (uintptr_t)1 << 32;
static void* take(size_t bytes, size_t off) {
  g_next = (g_next + 4095) & ~(uintptr_t)4095;
  const uintptr_t p = g_next + off;
  g_next = p + bytes + 256;
  return reinterpret_cast<void*>(p);
}

static size_t es_of(int dtype) { return dtype == kFloat64 ? 8 : dtype == kFloat32 ? 4 : 2; }

// nelem elements, the wide side `wide_off` BYTES and the fp16 side `half_off`
// BYTES past a 4-KiB boundary
static byteps_cast_desc seg(int dtype, size_t nelem, size_t wide_off = 0, size_t half_off = 0) {
  byteps_cast_desc d;
  d.wide = take(nelem * es_of(dtype), wide_off);
  d.half = take(nelem * 2, half_off);
  d.nelem = nelem;
  return d;
}

// Where the single cast's vector range lies, by brute force: the first
// element at which both operands are 16-byte aligned, if the operands are
// element-aligned and at least 8 elements follow it.
struct Want {
  bool aligned;
  uint64_t head, nunits;
};
static Want want_cut(const byteps_cast_desc& d, size_t es) {
  const uintptr_t w = (uintptr_t)d.wide, h = (uintptr_t)d.half;
  Want c{w % es == 0 && h % 2 == 0, 0, 0};
  if (!c.aligned) return c;
  for (uint64_t e = 0; e < 8 && e < d.nelem; ++e)  // the fp16 side repeats every 8 elements
    if ((w + e * es) % 16 == 0 && (h + e * 2) % 16 == 0) {
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

// Build and walk.  `want_u`: the tile size the rule must choose; `want_records`
// (if >= 0): the grid worked out by hand for the case.
static void accept(const std::string& name, const std::vector<byteps_cast_desc>& segs, int dtype,
                   int copy_vpt, int want_u, long want_records = -1) {
  g_case = name;
  const size_t es = es_of(dtype);
  std::vector<char> out(5, 'x');
  CastTableInfo ti;
  const int rc = build_cast_table(segs.data(), (int)segs.size(), dtype, copy_vpt, out, &ti);
  CHECK(rc == BYTEPS_REDUCE_OK, "rc %d (%s)", rc, g_msg.c_str());
  if (rc != BYTEPS_REDUCE_OK) return;
  std::vector<size_t> live;
  uint64_t total = 0;
  for (size_t i = 0; i < segs.size(); ++i)
    if (segs[i].nelem) live.push_back(i), total += segs[i].nelem;
  CHECK(ti.u == want_u, "u %d, want %d", ti.u, want_u);
  CHECK(ti.live == (int)live.size(), "live %d, want %zu", ti.live, live.size());
  CHECK(ti.nelem == total, "nelem %llu, want %llu", (unsigned long long)ti.nelem,
        (unsigned long long)total);
  CHECK(ti.bytes == out.size() && out.size() == (size_t)ti.records * sizeof(CastRec),
        "bytes %zu, out %zu, records %u", ti.bytes, out.size(), ti.records);
  if (want_records >= 0)
    CHECK(ti.records == (uint32_t)want_records, "records %u, want %ld", ti.records, want_records);
  if (out.size() != (size_t)ti.records * sizeof(CastRec) || (ti.u != 1 && ti.u != 2 && ti.u != 4))
    return;
  const uint64_t tile_units = (uint64_t)kBlock * (uint64_t)ti.u;
  // per live segment: 0 = not covered, 1 = element record, 2 = vector record
  std::vector<std::vector<unsigned char>> cover(live.size());
  std::vector<uintptr_t> last_full(live.size(), 0);
  for (size_t j = 0; j < live.size(); ++j) cover[j].assign(segs[live[j]].nelem, 0);
  uint64_t vec_tiles = 0;
  bool full_seen = false;
  for (uint32_t i = 0; i < ti.records; ++i) {
    const CastRec r = record(out, i);
    const uintptr_t w = (uintptr_t)r.wide;
    size_t j = live.size();
    for (size_t k = 0; k < live.size(); ++k) {
      const byteps_cast_desc& d = segs[live[k]];
      if (w >= (uintptr_t)d.wide && w < (uintptr_t)d.wide + d.nelem * es) j = k;
    }
    CHECK(j < live.size(), "record %u: wide pointer in no segment", i);
    if (j == live.size()) return;
    const byteps_cast_desc& d = segs[live[j]];
    const Want c = want_cut(d, es);
    const uint64_t wbytes = w - (uintptr_t)d.wide;
    CHECK(wbytes % es == 0, "record %u: %llu bytes into its segment", i,
          (unsigned long long)wbytes);
    const uint64_t first = wbytes / es;
    CHECK((uintptr_t)r.half == (uintptr_t)d.half + 2 * first, "record %u: fp16 pointer", i);
    CHECK(r.pad == 0, "record %u: pad %u", i, r.pad);
    uint64_t n = 0;
    unsigned char mark = 2;
    if (r.kind == kTileFull) {
      full_seen = true;
      n = 8 * tile_units;
      CHECK(r.count == tile_units, "record %u: full tile of %u units", i, r.count);
      CHECK(w > last_full[j], "record %u: full tiles of a segment out of address order", i);
      last_full[j] = w;
      ++vec_tiles;
    } else if (r.kind == kTilePartial) {
      CHECK(!full_seen, "record %u: guarded tile after a full tile", i);
      CHECK(r.count > 0 && r.count < tile_units, "record %u: guarded tile of %u units", i, r.count);
      n = 8 * (uint64_t)r.count;
      ++vec_tiles;
    } else {
      CHECK(r.kind == kTileElem, "record %u: kind %u", i, r.kind);
      CHECK(!full_seen, "record %u: element record after a full tile", i);
      CHECK(r.count > 0 && r.count <= kCastElemPart, "record %u: %u elements", i, r.count);
      CHECK(r.aligned == (c.aligned ? 1u : 0u), "record %u: aligned %u", i, r.aligned);
      n = r.count;
      mark = 1;
    }
    if (mark == 2)
      CHECK(w % 16 == 0 && (uintptr_t)r.half % 16 == 0, "record %u: vector tile not 16-B aligned",
            i);
    CHECK(first + n <= d.nelem, "record %u: elements [%llu, %llu) of %zu", i,
          (unsigned long long)first, (unsigned long long)(first + n), (size_t)d.nelem);
    if (first + n > d.nelem) return;
    for (uint64_t e = first; e < first + n; ++e) {
      CHECK(cover[j][e] == 0, "record %u: element %llu covered twice", i, (unsigned long long)e);
      cover[j][e] = mark;
    }
  }
  uint64_t want_tiles = 0;
  for (size_t j = 0; j < live.size(); ++j) {
    const byteps_cast_desc& d = segs[live[j]];
    const Want c = want_cut(d, es);
    want_tiles += (c.nunits + tile_units - 1) / tile_units;
    uint64_t bad = 0;
    for (uint64_t e = 0; e < d.nelem; ++e) {
      const bool vec = e >= c.head && e < c.head + 8 * c.nunits;
      if (cover[j][e] != (vec ? 2 : 1)) ++bad;
    }
    CHECK(bad == 0, "segment %zu: %llu elements not covered by the right kind of record", live[j],
          (unsigned long long)bad);
  }
  CHECK(vec_tiles == want_tiles, "%llu vector tiles, want %llu", (unsigned long long)vec_tiles,
        (unsigned long long)want_tiles);
  // the tile-size rule, from its definition
  auto tiles_at = [&](int u) {
    uint64_t t = 0;
    for (size_t j = 0; j < live.size(); ++j) {
      const uint64_t tu = (uint64_t)kBlock * (uint64_t)u;
      t += (want_cut(segs[live[j]], es).nunits + tu - 1) / tu;
    }
    return t;
  };
  int u = copy_vpt;
  while (u > 1 && tiles_at(u) < kMinTiles) u >>= 1;
  CHECK(ti.u == u, "u %d, the rule gives %d", ti.u, u);
}

static void reject(const std::string& name, const std::vector<byteps_cast_desc>& segs, int dtype,
                   int want_rc) {
  g_case = name;
  const std::vector<char> before(33, 'x');
  std::vector<char> out = before;
  CastTableInfo ti;
  const int rc = build_cast_table(segs.data(), (int)segs.size(), dtype, 2, out, &ti);
  CHECK(rc == want_rc && out == before, "rc %d, want %d, out %zu bytes", rc, want_rc, out.size());
}

int main() {
  const size_t kSizes[] = {0, 1, 7, 8, 9, 2047, 2048, 2049, 3 * 2048 + 5};
  const size_t kOffs[] = {0, 1, 3};  // elements
  for (int dtype : {kFloat32, kFloat64, kBFloat16}) {
    const size_t es = es_of(dtype);
    const std::string dn = dtype == kFloat32 ? "f32" : dtype == kFloat64 ? "f64" : "bf16";
    std::vector<byteps_cast_desc> all;
    // every size at every pair of offsets: with the fp16 side `oh` elements
    // and the wide side `ow` elements past a boundary the operands co-align
    // iff (8 - oh) % 8 = (16 / es - ow % (16 / es)) % (16 / es) mod 16 / es —
    // both kinds occur for every dtype
    for (size_t n : kSizes)
      for (size_t ow : kOffs)
        for (size_t oh : kOffs) {
          const byteps_cast_desc d = seg(dtype, n, ow * es, oh * 2);
          accept(dn + " n=" + std::to_string(n) + " ow=" + std::to_string(ow) + " oh=" +
                     std::to_string(oh),
                 {d}, dtype, 2, 1);
          all.push_back(d);
        }
    // element-misaligned operands: no vector range at all
    for (size_t n : {(size_t)9, (size_t)2049}) {
      const byteps_cast_desc a = seg(dtype, n, 1, 0), b = seg(dtype, n, 0, 1);
      accept(dn + " wide side element-misaligned", {a}, dtype, 2, 1, 1);
      accept(dn + " fp16 side element-misaligned", {b}, dtype, 2, 1, 1);
      all.push_back(a);
      all.push_back(b);
    }
    accept(dn + " all of the above in one plan", all, dtype, 2, 1);
    // a long segment that never co-aligns (fp16 side 2 bytes off) is split
    // into parts of kCastElemPart = 4096 elements: 24 whole parts and one more
    accept(dn + " 100000 elements, never co-aligning", {seg(dtype, 100000, 0, 2)}, dtype, 2, 1,
           25);
    // hand-counted: 3 * 2048 + 5 aligned elements are 3 full tiles at u = 1
    // and 5 tail elements in one element record
    accept(dn + " 3 tiles + 5", {seg(dtype, 3 * 2048 + 5)}, dtype, 2, 1, 4);
    // one tile + one unit: a full tile and a guarded tile of 1 unit
    accept(dn + " tile + unit", {seg(dtype, 2048 + 8)}, dtype, 2, 1, 2);
    // The tile size is chosen for the launch's total.  Segments of 32768
    // elements are 16 tiles at u = 1, 8 at u = 2, 4 at u = 4; kMinTiles =
    // 2048.  copy_vpt 4: 255 segments stay at u = 1 (2040 tiles at u = 2),
    // 256 reach u = 2, 511 stay there (2044 at u = 4), 512 reach u = 4.
    // copy_vpt 2 never exceeds 2, copy_vpt 1 never exceeds 1.
    std::vector<byteps_cast_desc> many;
    for (int k = 0; k < 512; ++k) many.push_back(seg(dtype, 32768));
    auto first = [&many](size_t n) {
      return std::vector<byteps_cast_desc>(many.begin(), many.begin() + (long)n);
    };
    accept(dn + " 255 segments", first(255), dtype, 4, 1, 255 * 16);
    accept(dn + " 256 segments", first(256), dtype, 4, 2, 256 * 8);
    accept(dn + " 511 segments", first(511), dtype, 4, 2, 511 * 8);
    accept(dn + " 512 segments", first(512), dtype, 4, 4, 512 * 4);
    accept(dn + " 512 segments, copy_vpt 2", first(512), dtype, 2, 2, 512 * 8);
    accept(dn + " 512 segments, copy_vpt 1", first(512), dtype, 1, 1, 512 * 16);
    {  // ... and with small odd segments among them, heads and tails at u = 4
      std::vector<byteps_cast_desc> mix = first(512);
      mix.push_back(seg(dtype, 3 * 2048 + 5, 3 * es, 6));
      mix.push_back(seg(dtype, 7));
      mix.push_back(seg(dtype, 0));
      mix.push_back(seg(dtype, 2049, 1, 0));
      accept(dn + " 512 segments and odd ones", mix, dtype, 4, 4);
    }
    // empty plans
    accept(dn + " no segments", {}, dtype, 2, 1, 0);
    {
      byteps_cast_desc z;
      z.wide = z.half = nullptr;
      z.nelem = 0;
      accept(dn + " only empty segments", {z, seg(dtype, 0), z}, dtype, 2, 1, 0);
    }
    // errors: nothing is written
    const byteps_cast_desc ok = seg(dtype, 64), ok2 = seg(dtype, 64);
    byteps_cast_desc b = ok2;
    b.wide = nullptr;
    reject(dn + " null wide", {ok, b}, dtype, BYTEPS_REDUCE_EARGS);
    b = ok2;
    b.half = nullptr;
    reject(dn + " null half", {ok, b}, dtype, BYTEPS_REDUCE_EARGS);
    b = ok2;
    b.wide = static_cast<char*>(ok.wide) + 8 * es;
    reject(dn + " wide overlaps wide", {ok, b}, dtype, BYTEPS_REDUCE_EARGS);
    reject(dn + " wide overlaps wide, other order", {b, ok}, dtype, BYTEPS_REDUCE_EARGS);
    b = ok2;
    b.half = static_cast<char*>(ok.half) + 126;
    reject(dn + " half overlaps half", {ok, b}, dtype, BYTEPS_REDUCE_EARGS);
    b = ok2;
    b.half = static_cast<char*>(ok.wide) + 64 * es - 2;
    reject(dn + " half overlaps another segment's wide", {ok, b}, dtype, BYTEPS_REDUCE_EARGS);
    b = ok2;
    b.wide = static_cast<char*>(ok.half) - 64 * es + 2;
    reject(dn + " wide overlaps another segment's half", {ok, b}, dtype, BYTEPS_REDUCE_EARGS);
    b = ok;
    b.half = ok.wide;
    reject(dn + " half is its own wide", {b}, dtype, BYTEPS_REDUCE_EARGS);
    b = seg(dtype, 4);
    b.wide = static_cast<char*>(ok.wide) + 16 * es;
    reject(dn + " a range inside another", {ok, ok2, b}, dtype, BYTEPS_REDUCE_EARGS);
    reject(dn + " a range inside another, other order", {b, ok2, ok}, dtype, BYTEPS_REDUCE_EARGS);
    reject(dn + " the same segment twice", {ok, ok2, ok}, dtype, BYTEPS_REDUCE_EARGS);
    // touching ranges are disjoint
    b = ok2;
    b.wide = static_cast<char*>(ok.wide) + 64 * es;
    accept(dn + " touching ranges", {ok, b}, dtype, 2, 1);
    // 2^43 elements that never co-align are 2^31 element records: too many
    b = seg(dtype, 8, 0, 2);
    b.nelem = (size_t)1 << 43;
    reject(dn + " grid of 2^31", {b}, dtype, BYTEPS_REDUCE_EARGS);
  }
  // the dtype comes first, and only the three wide types pass
  for (int dtype : std::vector<int>{kFloat16, kInt32, kUInt8, kInt8, kInt64, 7, -1})
    reject("dtype " + std::to_string(dtype), {}, dtype, BYTEPS_REDUCE_EDTYPE);
  {
    g_case = "null table";
    std::vector<char> out(3, 'x');
    CastTableInfo ti;
    CHECK(build_cast_table(nullptr, 2, kFloat32, 2, out, &ti) == BYTEPS_REDUCE_EARGS, "null segs");
    CHECK(build_cast_table(nullptr, -1, kFloat32, 2, out, &ti) == BYTEPS_REDUCE_EARGS, "nsegs < 0");
    CHECK(out == std::vector<char>(3, 'x'), "written");
  }
  printf("fails=%d\n", g_fails);
  return g_fails ? 1 : 0;
}
