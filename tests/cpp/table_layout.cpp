// CPU test of the batch-table builder (prophet_amd/csrc/bpsr_table.cpp, built
// unchanged by tests/test_table_layout.py, plain and under ASan + UBSan):
// every table it accepts is parsed back and compared with the layout that
// bpsr_internal.h defines (FoldGeom, BatchEntry, TileHead, kBlock), worked out
// here independently of make_geom / build_table.  The buffers are addresses
// inside one static arena; nothing is read or written through them.
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
Tuning launch_tuning_for_n(int n) {
  Tuning t{2, 1, 1 << 20, 1, 2, 0, 4096, 4096, 1, 4, 2, kWtMaxBytes};
  if (n <= 4) t.occ = 2, t.vpt = 4;
  return t;
}
}  // namespace bpsr

using namespace bpsr;

static int g_fails = 0;
static const char* g_case = "";
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      ++g_fails;                                           \
      printf("FAIL %s line %d: %s: ", g_case, __LINE__, #cond); \
      printf(__VA_ARGS__);                                 \
      printf("\n");                                        \
    }                                                      \
  } while (0)

alignas(4096) static unsigned char g_arena[4 << 20];
static size_t g_used = 0;
// `bytes` of the arena starting `off` bytes past a 256-B boundary
static unsigned char* take(size_t bytes, size_t off = 0) {
  g_used = (g_used + 255) & ~(size_t)255;
  unsigned char* p = g_arena + g_used + off;
  g_used += off + bytes + 64;
  if (g_used > sizeof(g_arena)) {
    printf("arena too small\n");
    std::exit(2);
  }
  return p;
}

static byteps_bucket_desc bucket(size_t len, int n, size_t dst_off = 0, size_t src_off = 0,
                                 int odd_src = -1, size_t odd_off = 0) {
  byteps_bucket_desc b;
  std::memset(&b, 0, sizeof(b));
  b.len = len;
  b.n = n;
  b.dst = take(len, dst_off);
  for (int k = 0; k < n; ++k) b.srcs[k] = take(len, k == odd_src ? odd_off : src_off);
  return b;
}

static int es_of(int dtype) {
  switch (dtype) {
    case kFloat16: case kBFloat16: return 2;
    case kFloat32: case kInt32: return 4;
    case kFloat64: case kInt64: return 8;
    default: return 1;
  }
}

// The geometry of one bucket from the definitions of FoldGeom's fields.
struct Geom {
  uint64_t n_elems, head, vec_off, nvec, tail_begin, tail_sem_from, trailing, parts;
  uint32_t copy_trailing;
  int aligned;
};
static Geom expect_geom(const byteps_bucket_desc& b, int dtype) {
  const uint64_t es = (uint64_t)es_of(dtype);
  const uintptr_t d = (uintptr_t)b.dst;
  Geom g{};
  g.n_elems = b.len / es;
  g.trailing = b.len % es;
  g.copy_trailing = (b.dst != b.srcs[0] && g.trailing) ? 1u : 0u;
  bool vec_ok = d % es == 0;  // every operand element-aligned and at dst's offset mod 16
  g.aligned = d % es == 0;
  for (int k = 0; k < b.n; ++k) {
    const uintptr_t s = (uintptr_t)b.srcs[k];
    if (s % es) g.aligned = 0;
    vec_ok = vec_ok && s % es == 0 && s % 16 == d % 16;
  }
  // fp16: the last n_elems % 8 elements keep the scalar tail's semantics
  const uint64_t body = dtype == kFloat16 ? g.n_elems - g.n_elems % 8 : g.n_elems;
  g.tail_sem_from = body;
  if (vec_ok) {
    g.head = (d % 16 ? 16 - d % 16 : 0) / es;
    if (g.head > g.n_elems) g.head = g.n_elems;
    g.vec_off = g.head * es;
    g.nvec = body > g.head ? (body - g.head) * es / 16 : 0;
    g.tail_begin = g.head + g.nvec * 16 / es;
  }
  const uint64_t scalar = g.head + g.n_elems - g.tail_begin;
  const uint64_t part = (uint64_t)kBlock * 16;  // elements per element tile
  g.parts = (scalar || g.copy_trailing) ? (scalar + part - 1) / part : 0;
  if ((scalar || g.copy_trailing) && g.parts < 1) g.parts = 1;
  return g;
}

struct Rec {
  TileHead h;
  const unsigned char* src[kMaxSrcs];
};
static Rec record(const std::vector<char>& out, const TableInfo& ti, uint32_t i) {
  Rec r;
  const char* p = out.data() + ti.recs_off + (size_t)ti.rec_stride * i;
  std::memcpy(&r.h, p, sizeof(r.h));
  std::memset(r.src, 0, sizeof(r.src));
  std::memcpy(r.src, p + kTileHeadBytes, ti.rec_stride - kTileHeadBytes);
  return r;
}

// Build the table and check every invariant of an accepted one.  `want_vpt`:
// the tile size the fold rule must choose (or force_vpt); `want_tiles`: the
// record count worked out by hand for the case.
static void accept(const char* name, const std::vector<byteps_bucket_desc>& bk, int dtype,
                   const std::vector<int>& block_end, int force_vpt, int want_vpt,
                   uint32_t want_tiles, std::vector<char>* table = nullptr) {
  g_case = name;
  const int nb = (int)bk.size(), nblocks = (int)block_end.size();
  std::vector<char> out(7, 'x');
  std::vector<uint32_t> bf;
  TableInfo ti;
  const int rc = nblocks ? build_table(bk.data(), nb, dtype, out, &ti, block_end.data(), nblocks,
                                       &bf, force_vpt)
                         : build_table(bk.data(), nb, dtype, out, &ti, nullptr, 0, nullptr,
                                       force_vpt);
  CHECK(rc == BYTEPS_REDUCE_OK, "rc %d (%s)", rc, g_msg.c_str());
  if (rc != BYTEPS_REDUCE_OK) return;
  // the live buckets, their blocks and their geometry
  std::vector<int> live, live_block;
  std::vector<Geom> geom;
  int nmax = 1;
  for (int i = 0, blk = 0; i < nb; ++i) {
    while (blk < nblocks && i >= block_end[(size_t)blk]) ++blk;
    if (bk[(size_t)i].len == 0) continue;
    live.push_back(i);
    live_block.push_back(blk);
    geom.push_back(expect_geom(bk[(size_t)i], dtype));
    if (bk[(size_t)i].n > nmax) nmax = bk[(size_t)i].n;
  }
  const uint32_t stride = (32u + 8u * (uint32_t)(nmax < 8 ? 8 : nmax) + 31u) & ~31u;
  const uint64_t tile_vecs = (uint64_t)kBlock * (uint64_t)want_vpt;
  uint64_t tiles = 0;
  for (const Geom& g : geom) tiles += g.parts + (g.nvec + tile_vecs - 1) / tile_vecs;
  CHECK(ti.vpt == want_vpt, "vpt %d, want %d", ti.vpt, want_vpt);
  CHECK(ti.nmax == nmax, "nmax %d, want %d", ti.nmax, nmax);
  CHECK(ti.live == (int)live.size(), "live %d, want %zu", ti.live, live.size());
  CHECK(ti.tiles == want_tiles && tiles == want_tiles, "tiles %u, model %llu, want %u", ti.tiles,
        (unsigned long long)tiles, want_tiles);
  CHECK(ti.rec_stride == stride && stride == tile_rec_stride(nmax), "stride %u, want %u",
        ti.rec_stride, stride);
  CHECK(ti.recs_off % 256 == 0 && ti.recs_off >= sizeof(BatchEntry) * live.size() &&
            ti.recs_off < sizeof(BatchEntry) * live.size() + 256,
        "recs_off %zu for %zu entries", ti.recs_off, live.size());
  CHECK(ti.bytes == out.size() && ti.bytes == ti.recs_off + (size_t)stride * ti.tiles,
        "bytes %zu, out %zu", ti.bytes, out.size());
  if (ti.bytes != out.size() || ti.bytes != ti.recs_off + (size_t)stride * ti.tiles ||
      ti.live != (int)live.size() || ti.rec_stride != stride)
    return;
  // the BatchEntry of every live bucket
  for (size_t j = 0; j < live.size(); ++j) {
    const byteps_bucket_desc& b = bk[(size_t)live[j]];
    const Geom& g = geom[j];
    BatchEntry e;
    std::memcpy(&e, out.data() + sizeof(e) * j, sizeof(e));
    CHECK(e.dst == b.dst && e.n == b.n && e.aligned == g.aligned, "entry %zu: n %d aligned %d", j,
          e.n, e.aligned);
    for (int k = 0; k < kMaxSrcs; ++k)
      CHECK(e.srcs[k] == (k < b.n ? b.srcs[k] : nullptr), "entry %zu: srcs[%d]", j, k);
    CHECK(e.g.n_elems == g.n_elems && e.g.head_elems == g.head && e.g.vec_off == g.vec_off &&
              e.g.nvec == g.nvec && e.g.tail_begin == g.tail_begin &&
              e.g.tail_sem_from == g.tail_sem_from && e.g.trailing_bytes == g.trailing &&
              e.g.copy_trailing == g.copy_trailing,
          "entry %zu: geometry (nvec %llu, want %llu)", j, (unsigned long long)e.g.nvec,
          (unsigned long long)g.nvec);
  }
  // the records, in order
  std::vector<uint64_t> next_part(live.size(), 0), next_vec(live.size(), 0);
  if (nblocks) {
    CHECK(bf.size() == (size_t)nblocks + 1 && bf[0] == 0 && bf[(size_t)nblocks] == ti.tiles,
          "block_first: %zu entries", bf.size());
    if (bf.size() != (size_t)nblocks + 1) return;
    for (int k = 0; k < nblocks; ++k)
      CHECK(bf[(size_t)k] <= bf[(size_t)k + 1], "block_first[%d] %u > %u", k, bf[(size_t)k],
            bf[(size_t)k + 1]);
  }
  uint32_t blk = 0;
  bool vec_seen = false;  // in the current block
  for (uint32_t i = 0; i < ti.tiles; ++i) {
    const Rec r = record(out, ti, i);
    while (nblocks && blk + 1 < (uint32_t)nblocks && i >= bf[blk + 1]) ++blk, vec_seen = false;
    CHECK(r.h.block == blk, "record %u: block %u, want %u", i, r.h.block, blk);
    CHECK(r.h.b < live.size(), "record %u: bucket %u", i, r.h.b);
    if (r.h.b >= live.size()) return;
    const size_t j = r.h.b;
    const byteps_bucket_desc& b = bk[(size_t)live[j]];
    const Geom& g = geom[j];
    if (nblocks) CHECK(live_block[j] == (int)blk, "record %u: bucket of block %d", i, live_block[j]);
    CHECK(r.h.n == (uint32_t)b.n, "record %u: n %u", i, r.h.n);
    const ptrdiff_t at = r.h.dst - static_cast<unsigned char*>(b.dst);
    for (int k = 0; k < (int)((stride - kTileHeadBytes) / 8); ++k)
      CHECK(r.src[k] == (k < b.n ? static_cast<const unsigned char*>(b.srcs[k]) + at : nullptr),
            "record %u: source %d", i, k);
    if (r.h.kind == kTileElem) {
      CHECK(!vec_seen, "record %u: element tile after a vector tile of its block", i);
      CHECK(at == 0 && r.h.c == g.parts && r.h.a == next_part[j], "record %u: part %u of %u", i,
            r.h.a, r.h.c);
      ++next_part[j];
      continue;
    }
    vec_seen = true;
    const uint64_t left = g.nvec - next_vec[j];
    CHECK(next_vec[j] < g.nvec && at == (ptrdiff_t)(g.vec_off + 16 * next_vec[j]),
          "record %u: vector tile at byte %td", i, at);
    if (left >= tile_vecs) {
      CHECK(r.h.kind == kTileFull && r.h.a == 0, "record %u: kind %u a %u", i, r.h.kind, r.h.a);
      next_vec[j] += tile_vecs;
    } else {  // only a bucket's last tile, with the remainder
      CHECK(r.h.kind == kTilePartial && r.h.a == left, "record %u: kind %u a %u, %llu left", i,
            r.h.kind, r.h.a, (unsigned long long)left);
      next_vec[j] = g.nvec;
    }
  }
  for (size_t j = 0; j < live.size(); ++j)
    CHECK(next_part[j] == geom[j].parts && next_vec[j] == geom[j].nvec,
          "bucket %zu: %llu parts, %llu vectors covered", j, (unsigned long long)next_part[j],
          (unsigned long long)next_vec[j]);
  if (table) *table = out;
  if (!nblocks) {  // the same bytes as one block of all the buckets
    std::vector<char> one;
    accept(name, bk, dtype, {nb}, force_vpt, want_vpt, want_tiles, &one);
    g_case = name;
    CHECK(one == out, "differs from the one-block table");
  }
}

static void reject(const char* name, const std::vector<byteps_bucket_desc>& bk) {
  g_case = name;
  const std::vector<char> before(33, 'x');
  std::vector<char> out = before;
  std::vector<uint32_t> bf;
  const int end = (int)bk.size();
  TableInfo ti;
  int rc = build_table(bk.data(), end, kFloat32, out, &ti);
  CHECK(rc == BYTEPS_REDUCE_EARGS && out == before, "rc %d, out %zu bytes", rc, out.size());
  rc = build_table(bk.data(), end, kFloat32, out, &ti, &end, 1, &bf);
  CHECK(rc == BYTEPS_REDUCE_EARGS && out == before && bf.empty(), "blocks: rc %d", rc);
}

int main() {
  const size_t kTile = (size_t)kBlock * 16;  // bytes of a tile at vpt 1
  // one full tile plus one vector: a full and a partial tile with a = 1
  accept("f32 tile+vector", {bucket(kTile + 16, 2)}, kFloat32, {}, 0, 1, 2);
  // dst and sources 4 bytes past a 16-B boundary: 3 head elements and 1 tail
  // element in one element tile, 256 vectors in one full tile
  accept("f32 head", {bucket(kTile + 16, 2, 4, 4)}, kFloat32, {}, 0, 1, 2);
  // one source 2 bytes off: no vector range, 1028 elements in one element tile
  accept("f32 misaligned source", {bucket(kTile + 16, 2, 4, 4, 1, 6)}, kFloat32, {}, 0, 1, 1);
  // fp16, 8 * 40 + 3 elements: 40 vectors, the 3 tail elements apart
  accept("f16 tail", {bucket(2 * 323, 2)}, kFloat16, {}, 0, 1, 2);
  {  // ... and a trailing odd byte: copied when dst is not srcs[0], else left alone
    byteps_bucket_desc b = bucket(2 * 320 + 1, 2);
    accept("f16 trailing byte", {b}, kFloat16, {}, 0, 1, 2);
    b.srcs[0] = b.dst;
    accept("f16 trailing byte in place", {b}, kFloat16, {}, 0, 1, 1);
  }
  accept("one source", {bucket(kTile + 16, 1)}, kFloat32, {}, 0, 1, 2);
  accept("kMaxSrcs sources", {bucket(kTile + 16, kMaxSrcs)}, kFloat32, {}, 0, 1, 2);
  {  // three blocks: [head + tile, empty, tail + tile], [empty], [one tile]
    const std::vector<byteps_bucket_desc> bk = {bucket(kTile + 16, 2, 4, 4), bucket(0, 3),
                                                bucket(kTile + 4, 2), bucket(0, 2),
                                                bucket(kTile, 9)};
    accept("blocks", bk, kFloat32, {3, 4, 5}, 0, 1, 5);
    accept("blocks as one launch", bk, kFloat32, {}, 0, 1, 5);
  }
  {  // three tiles at vpt 1: 3 full; 1 full + 1 partial (256); 1 partial (768)
    const std::vector<byteps_bucket_desc> bk = {bucket(3 * kTile, 2), bucket(3 * kTile, 2)};
    const uint32_t per_bucket[5] = {0, 3, 2, 0, 1};
    for (int vpt : {1, 2, 4}) {
      accept("force_vpt, two blocks", bk, kFloat32, {1, 2}, vpt, vpt, 2 * per_bucket[vpt]);
      accept("force_vpt, no blocks", bk, kFloat32, {}, vpt, vpt, 2 * per_bucket[vpt]);
    }
  }
  {
    const byteps_bucket_desc ok = bucket(64, 2);
    byteps_bucket_desc b = ok;
    b.n = 0;
    reject("n = 0", {ok, b});
    b.n = kMaxSrcs + 1;
    reject("n = kMaxSrcs + 1", {ok, b});
    b = ok;
    b.dst = nullptr;
    reject("null dst", {ok, b});
    b = ok;
    b.srcs[1] = nullptr;
    reject("null source", {ok, b});
    b = ok;
    b.srcs[0] = static_cast<unsigned char*>(b.dst) + 8;
    reject("partial overlap", {ok, b});
    b = ok;
    b.srcs[1] = b.dst;
    reject("srcs[1] == dst", {ok, b});
  }
  printf("fails=%d\n", g_fails);
  return g_fails ? 1 : 0;
}
