// What the cast launch rules make of the shapes of tests/cast_shapes.py: the
// host arithmetic of prophet_amd/csrc/bpsr_internal.h (cast_cut, cache_pol)
// and bpsr_cast_table.cpp (build_cast_table, build_cast_table_ef), compiled
// unchanged with g++ by tests/test_cast_shapes.py.  Reads cases from stdin:
//
//   plan <es> <copy_vpt> <wt_max_mib> <ef> <nsegs>
//   s <nelem> <wide offset> <half offset>                     (nsegs lines)
//     one cast plan (ef = 1: an error-feedback plan, the residuals laid out
//     like the wide operands) whose operands lie at these byte offsets in one
//     256-byte aligned arena a side; wt_max_mib < 0 is the default.  A
//     one-tensor call is a plan of one segment: cast_rule (bpsr_cast_single.h)
//     applies the same cut and the same halving loop to its one operand pair.
//
// and prints for the plan
//   plan u= records= pol_c= pol_d= pol_ef=
//     CastTableInfo::u, and the store policy (cache_pol with nt = 1, which is
//     cast_store_pol) of the bytes a compress, a decompress and an
//     error-feedback compress of the plan write, as cast_plan_launch and
//     launch_cast count them
// and for every segment, from its record list (CastSegList),
//   seg full= partial= pcount= head= tail= elem=
//     its kTileFull and kTilePartial records, the last partial record's
//     count, the counts of the kTileElem records at its first element and
//     behind its vector range (0: none), and all its kTileElem records.
//
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

static const uintptr_t kArena[3] = {(uintptr_t)1 << 40, (uintptr_t)2 << 40, (uintptr_t)3 << 40};

static int do_plan(const char* line) {
  int es, copy_vpt, ef, nsegs;
  long wt;
  if (sscanf(line, "plan %d %d %ld %d %d", &es, &copy_vpt, &wt, &ef, &nsegs) != 5) return 2;
  if ((es != 2 && es != 4 && es != 8) || nsegs < 1 || (ef && es != 4)) return 2;
  const int dtype = es == 8 ? kFloat64 : es == 4 ? kFloat32 : kBFloat16;
  std::vector<byteps_cast_desc> d((size_t)nsegs);
  std::vector<byteps_cast_ef_desc> de((size_t)nsegs);
  char buf[256];
  for (int i = 0; i < nsegs; ++i) {
    unsigned long long n, wo, ho;
    if (!fgets(buf, sizeof(buf), stdin) || sscanf(buf, "s %llu %llu %llu", &n, &wo, &ho) != 3)
      return 2;
    d[(size_t)i] = {reinterpret_cast<void*>(kArena[0] + wo), reinterpret_cast<void*>(kArena[1] + ho),
                    (size_t)n};
    de[(size_t)i] = {d[(size_t)i].wide, d[(size_t)i].half,
                     reinterpret_cast<void*>(kArena[2] + wo), (size_t)n};
  }
  std::vector<char> out;
  std::vector<unsigned char*> resid;
  CastTableInfo ti;
  CastSegList l;
  const int rc = ef ? build_cast_table_ef(de.data(), nsegs, dtype, copy_vpt, out, resid, &ti, &l)
                    : build_cast_table(d.data(), nsegs, dtype, copy_vpt, out, &ti, &l);
  if (rc != BYTEPS_REDUCE_OK) {
    printf("error %d %s\n", rc, g_msg.c_str());
    return 1;
  }
  Tuning tu = launch_tuning_for_n(0);
  tu.nt = 1;  // cast_store_pol
  if (wt >= 0) tu.wt_max_bytes = (uint64_t)wt << 20;
  printf("plan u=%d records=%u pol_c=%d pol_d=%d pol_ef=%d\n", ti.u, ti.records,
         cache_pol(tu, ti.nelem * 2), cache_pol(tu, ti.nelem * (uint64_t)es),
         cache_pol(tu, ti.nelem * 6));
  if (l.seg_begin.size() != (size_t)nsegs + 1) return 3;
  for (int i = 0; i < nsegs; ++i) {
    unsigned long long full = 0, partial = 0, pcount = 0, head = 0, tail = 0, elem = 0;
    const uintptr_t w0 = (uintptr_t)d[(size_t)i].wide;
    for (uint32_t k = l.seg_begin[(size_t)i]; k < l.seg_begin[(size_t)i + 1]; ++k) {
      CastRec r;
      std::memcpy(&r, out.data() + (size_t)l.seg_recs[k] * sizeof(CastRec), sizeof(r));
      const unsigned long long first = ((uintptr_t)r.wide - w0) / (unsigned)es;
      if (r.kind == kTileFull) {
        if (r.count != (uint32_t)kBlock * (uint32_t)ti.u) return 4;
        ++full;
      } else if (r.kind == kTilePartial) {
        ++partial;
        pcount = r.count;
      } else if (r.kind == kTileElem) {
        ++elem;
        if (first == 0) head = r.count;
        else if (first + r.count == d[(size_t)i].nelem) tail = r.count;
      } else {
        return 4;
      }
    }
    printf("seg full=%llu partial=%llu pcount=%llu head=%llu tail=%llu elem=%llu\n", full, partial,
           pcount, head, tail, elem);
  }
  return 0;
}

int main() {
  char line[256];
  while (fgets(line, sizeof(line), stdin)) {
    int rc = 2;
    if (!std::strncmp(line, "plan ", 5)) rc = do_plan(line);
    else if (line[0] == '\n' || line[0] == '#') continue;
    if (rc) {
      printf("bad case (%d): %s", rc, line);
      return rc;
    }
  }
  printf("done\n");
  return 0;
}
