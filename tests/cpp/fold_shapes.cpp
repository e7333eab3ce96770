// What the launch rules make of the shapes of tests/fold_shapes.py: the host
// arithmetic of prophet_amd/csrc/bpsr_internal.h (fold_vpt, cache_pol) and
// bpsr_table.cpp (make_geom, build_table), compiled unchanged with g++ by
// tests/test_fold_shapes.py.  Reads cases from stdin, prints one line each:
//
//   fold <dtype> <n_elems> <n_src> <offset> <nt> <wt_max_mib>
//     one byteps_reduce_sum_n, every operand <offset> bytes past a 16-byte
//     boundary -> vpt (fold_vpt of the tuned tile size), pol (cache_pol),
//     band (1: launch_fold_op's half-tile band, from kHalfTileMinBytes per
//     source), nvec, head, full tiles and the partial tile's vectors
//   table <dtype> <nt> <wt_max_mib> <force_vpt> <blocks> <nbuckets>
//   b <len> <n> <block> <dst offset> <source offsets ...>      (nbuckets lines)
//     one batched / planned / block-queue table -> TableInfo.vpt, nmax, tiles,
//     pol, and the records counted by kind and by path (n <= 8: register
//     path, n > 8: pointer array)
//
// The buffers are made-up addresses; nothing is read or written through them.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bpsr_api_internal.h"

namespace bpsr {
// stand-ins for bpsr_api.cpp (HIP): the error text and the tuning
static std::string g_msg;
static int g_nt = 1;
static uint64_t g_wt_max = kWtMaxBytes;
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
  Tuning t{2, g_nt, 1 << 20, 1, 2, 0, 4096, 4096, 1, 4, 2, g_wt_max};
  if (n <= 4) t.occ = 2, t.vpt = 4;
  return t;
}
}  // namespace bpsr

using namespace bpsr;

static uintptr_t g_next = (uintptr_t)1 << 32;
// `bytes` of address space `off` bytes past a 256-B boundary
static unsigned char* take(size_t bytes, size_t off) {
  g_next = (g_next + 255) & ~(uintptr_t)255;
  const uintptr_t p = g_next + off;
  g_next += off + bytes + 64;
  return reinterpret_cast<unsigned char*>(p);
}

static void set_tuning(int nt, long wt_mib) {
  g_nt = nt ? 1 : 0;
  g_wt_max = wt_mib < 0 ? kWtMaxBytes : (uint64_t)wt_mib << 20;
}

static int do_fold(const char* line) {
  int dtype, n, off, nt;
  unsigned long long ne;
  long wt;
  if (sscanf(line, "fold %d %llu %d %d %d %ld", &dtype, &ne, &n, &off, &nt, &wt) != 6) return 2;
  if (n < 1 || n > kMaxSrcs || elem_size(dtype) == 0) return 2;
  set_tuning(nt, wt);
  const size_t len = (size_t)ne * (size_t)elem_size(dtype);
  const void* srcs[kMaxSrcs];
  for (int k = 0; k < n; ++k) srcs[k] = take(len, (size_t)off);
  void* dst = take(len, (size_t)off);
  FoldGeom g;
  int aligned = 0;
  make_geom(dtype, len, dst, srcs, n, true, &g, &aligned);
  const Tuning tu = launch_tuning_for_n(n);
  const int vpt = fold_vpt(g.nvec, tu.vpt);
  const int pol = cache_pol(tu, g.nvec * 16);
  const int band = pol == kPolWt && vpt == 2 && tu.occ == 1 && g.nvec * 16 >= kHalfTileMinBytes;
  const uint64_t tile = (uint64_t)kBlock * (uint64_t)vpt;
  printf("fold vpt=%d pol=%d band=%d nvec=%llu head=%llu tail=%llu full=%llu partial=%llu "
         "grid=%d aligned=%d\n",
         vpt, pol, band, (unsigned long long)g.nvec, (unsigned long long)g.head_elems,
         (unsigned long long)(g.n_elems - g.tail_begin), (unsigned long long)(g.nvec / tile),
         (unsigned long long)(g.nvec % tile), fold_grid(g, tu, vpt), aligned);
  return 0;
}

static int do_table(const char* line) {
  int dtype, nt, force_vpt, nblocks, nb;
  long wt;
  if (sscanf(line, "table %d %d %ld %d %d %d", &dtype, &nt, &wt, &force_vpt, &nblocks, &nb) != 6)
    return 2;
  if (nb < 0 || nblocks < 0 || elem_size(dtype) == 0) return 2;
  set_tuning(nt, wt);
  std::vector<byteps_bucket_desc> bk((size_t)nb);
  std::vector<int> block_end((size_t)nblocks, 0);
  char buf[1024];
  for (int i = 0; i < nb; ++i) {
    if (!fgets(buf, sizeof(buf), stdin)) return 2;
    unsigned long long len;
    int n, block, used = 0, doff;
    if (sscanf(buf, "b %llu %d %d %d%n", &len, &n, &block, &doff, &used) != 4) return 2;
    if (n < 1 || n > kMaxSrcs || (nblocks && (block < 0 || block >= nblocks))) return 2;
    byteps_bucket_desc& b = bk[(size_t)i];
    std::memset(&b, 0, sizeof(b));
    b.len = (size_t)len;
    b.n = n;
    b.dst = take((size_t)len, (size_t)doff);
    const char* p = buf + used;
    for (int k = 0; k < n; ++k) {
      int soff, u = 0;
      if (sscanf(p, "%d%n", &soff, &u) != 1) return 2;
      p += u;
      b.srcs[k] = take((size_t)len, (size_t)soff);
    }
    for (int k = block; nblocks && k < nblocks; ++k) block_end[(size_t)k] = i + 1;
  }
  std::vector<char> out;
  std::vector<uint32_t> bf;
  TableInfo ti;
  const int rc = nblocks ? build_table(bk.data(), nb, dtype, out, &ti, block_end.data(), nblocks,
                                       &bf, force_vpt)
                         : build_table(bk.data(), nb, dtype, out, &ti, nullptr, 0, nullptr,
                                       force_vpt);
  if (rc != BYTEPS_REDUCE_OK) {
    printf("error %d %s\n", rc, g_msg.c_str());
    return 1;
  }
  unsigned long long cnt[3][2] = {{0, 0}, {0, 0}, {0, 0}};
  for (uint32_t i = 0; i < ti.tiles; ++i) {
    TileHead h;
    std::memcpy(&h, out.data() + ti.recs_off + (size_t)ti.rec_stride * i, sizeof(h));
    if (h.kind > kTileElem) return 3;
    ++cnt[h.kind][h.n > 8 ? 1 : 0];
  }
  const int pol = cache_pol(launch_tuning_for_n(ti.nmax),
                            (uint64_t)ti.tiles * (uint64_t)ti.vpt * kBlock * 16);
  printf("table vpt=%d nmax=%d tiles=%u pol=%d full_reg=%llu full_mem=%llu partial_reg=%llu "
         "partial_mem=%llu elem=%llu\n",
         ti.vpt, ti.nmax, ti.tiles, pol, cnt[kTileFull][0], cnt[kTileFull][1],
         cnt[kTilePartial][0], cnt[kTilePartial][1], cnt[kTileElem][0] + cnt[kTileElem][1]);
  return 0;
}

int main() {
  char line[1024];
  while (fgets(line, sizeof(line), stdin)) {
    int rc = 2;
    if (!std::strncmp(line, "fold ", 5)) rc = do_fold(line);
    else if (!std::strncmp(line, "table ", 6)) rc = do_table(line);
    else if (line[0] == '\n' || line[0] == '#') continue;
    if (rc) {
      printf("bad case (%d): %s", rc, line);
      return rc;
    }
  }
  printf("done\n");
  return 0;
}
