// CPU test of the single casts' operand check (cast_check,
// prophet_amd/csrc/bpsr_cast_table.cpp, built unchanged by
// tests/test_cast_check.py, plain and under ASan + UBSan).  For every scheme
// (plain, error feedback, stochastic rounding) and both wire formats: every
// (wide, wire) dtype pair, nelem == 0, each null operand, an element count
// that overflows the byte count, each operand wrapping the address space, and
// for every pair of operands an overlap by one byte (rejected) and exact
// adjacency (accepted), each with its status and message text.  The operands
// are made-up addresses; nothing is read or written through them.
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

static int g_fails = 0, g_cases = 0;
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

static const char* const kSchemeName[3] = {"plain", "ef", "sr"};
static const char* wire_name(int wire) { return wire == kFloat16 ? "fp16" : "bf16"; }

// The operands of a cast of `scheme` whose wide side has `es`-byte elements,
// as the C entries name them; all null.
static std::vector<CastOperand> operands(CastScheme scheme, size_t es) {
  if (scheme == kCastEf) return {{"dst", nullptr, 2}, {"resid", nullptr, 4}, {"src", nullptr, 4}};
  return {{"dst", nullptr, 2}, {"src", nullptr, es}};
}

// ... `nelem` elements each, at made-up addresses a gap apart
static std::vector<CastOperand> placed(CastScheme scheme, size_t es, size_t nelem) {
  std::vector<CastOperand> ops = operands(scheme, es);
  uintptr_t at = (uintptr_t)1 << 32;
  for (CastOperand& o : ops) {
    o.p = reinterpret_cast<const void*>(at);
    at += nelem * o.es + 4096;
  }
  return ops;
}

// want_msg null: accepted (want_rc 0, or 1 for "nothing to do")
static void expect(const std::string& name, int wire, int wide, CastScheme scheme, int divisor,
                   size_t nelem, const std::vector<CastOperand>& ops, int want_rc,
                   const char* want_msg) {
  g_case = std::string(kSchemeName[scheme]) + " wire " + std::to_string(wire) + ": " + name;
  ++g_cases;
  g_msg = "(no message)";
  const int rc = cast_check(wire, wide, scheme, divisor, nelem, ops.data(), (int)ops.size());
  CHECK(rc == want_rc, "rc %d, want %d (%s)", rc, want_rc, g_msg.c_str());
  if (want_msg) CHECK(g_msg == want_msg, "message \"%s\", want \"%s\"", g_msg.c_str(), want_msg);
}

static std::string fmt(const char* f, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}

static size_t es_of(int dtype) { return dtype == kFloat64 ? 8 : dtype == kFloat32 ? 4 : 2; }

int main() {
  const int all_dtypes[] = {kFloat32, kFloat64, kFloat16, kUInt8, kInt32, kInt8, kInt64,
                            kBFloat16, 7, 99, -1};
  for (CastScheme scheme : {kCastPlain, kCastEf, kCastSr}) {
    // a wire format that is none: the first test, whatever the wide dtype
    for (int wire : {(int)kFloat32, (int)kFloat64, (int)kUInt8, 99, -1})
      for (int wide : all_dtypes)
        expect("wire, wide " + std::to_string(wide), wire, wide, scheme, 1, 100,
               placed(scheme, 4, 100), BYTEPS_REDUCE_EDTYPE,
               fmt("compression to data type %d", wire).c_str());
    for (int wire : {(int)kFloat16, (int)kBFloat16}) {
      // every (wide, wire) pair
      std::vector<int> wides;
      for (int wide : all_dtypes) {
        const int other = wire == kFloat16 ? kBFloat16 : kFloat16;
        const bool ok = scheme == kCastPlain
                            ? wide == kFloat32 || wide == kFloat64 || wide == other
                            : wide == kFloat32;
        const std::string msg =
            scheme == kCastPlain
                ? fmt("%s compression of data type %d", wire_name(wire), wide)
                : fmt("%s compression of data type %d (FLOAT32 only)",
                      scheme == kCastEf ? "error-feedback" : "stochastic-rounding", wide);
        if (ok) wides.push_back(wide);
        expect("pair, wide " + std::to_string(wide), wire, wide, scheme, 1, 100,
               placed(scheme, es_of(wide), 100), ok ? BYTEPS_REDUCE_OK : BYTEPS_REDUCE_EDTYPE,
               ok ? nullptr : msg.c_str());
        // the dtype error comes before every other, "nothing to do" included
        if (!ok)
          expect("pair before nelem 0, wide " + std::to_string(wide), wire, wide, scheme, 0, 0,
                 operands(scheme, es_of(wide)), BYTEPS_REDUCE_EDTYPE, msg.c_str());
      }
      CHECK(wides.size() == (scheme == kCastPlain ? 3u : 1u), "%zu accepted wide dtypes",
            wides.size());
      for (int wide : wides) {
        const size_t es = es_of(wide);
        const std::string w = ", wide " + std::to_string(wide);
        // the divisor (a decompress's; a compress passes 1), then nelem == 0
        expect("divisor 0" + w, wire, wide, scheme, 0, 100, placed(scheme, es, 100),
               BYTEPS_REDUCE_EARGS, "divisor 0 < 1");
        expect("divisor -3, nelem 0" + w, wire, wide, scheme, -3, 0, operands(scheme, es),
               BYTEPS_REDUCE_EARGS, "divisor -3 < 1");
        expect("divisor 7" + w, wire, wide, scheme, 7, 100, placed(scheme, es, 100),
               BYTEPS_REDUCE_OK, nullptr);
        expect("nelem 0, null operands" + w, wire, wide, scheme, 1, 0, operands(scheme, es), 1,
               nullptr);
        {
          // ... and overlapping ones: nothing is touched
          std::vector<CastOperand> ops = placed(scheme, es, 100);
          for (CastOperand& o : ops) o.p = ops[0].p;
          expect("nelem 0, one address" + w, wire, wide, scheme, 1, 0, ops, 1, nullptr);
        }
        const size_t nops = operands(scheme, es).size();
        for (size_t i = 0; i < nops; ++i) {
          std::vector<CastOperand> ops = placed(scheme, es, 100);
          const std::string who = std::string(ops[i].name) + w;
          ops[i].p = nullptr;
          expect("null " + who, wire, wide, scheme, 1, 100, ops, BYTEPS_REDUCE_EARGS,
                 "null pointer");
          // an operand whose last byte would lie past the address space, and
          // the furthest one that fits
          ops = placed(scheme, es, 100);
          ops[i].p = reinterpret_cast<const void*>(UINTPTR_MAX - 100 * ops[i].es + 1);
          expect("wrap " + who, wire, wide, scheme, 1, 100, ops, BYTEPS_REDUCE_EARGS,
                 "operand wraps the address space");
          ops[i].p = reinterpret_cast<const void*>(UINTPTR_MAX - 100 * ops[i].es);
          expect("ends at the top " + who, wire, wide, scheme, 1, 100, ops, BYTEPS_REDUCE_OK,
                 nullptr);
        }
        // an element count whose byte count overflows (stochastic rounding
        // refuses it by its own, lower limit)
        for (size_t n : {SIZE_MAX / es + 1, (size_t)SIZE_MAX})
          expect("nelem " + std::to_string(n) + w, wire, wide, scheme, 1, n,
                 placed(scheme, es, 100), BYTEPS_REDUCE_EARGS,
                 scheme == kCastSr ? "more than 2^34 elements" : "element count overflows");
        // every pair of operands: one byte shared from either side is an
        // overlap, exact adjacency is none
        const size_t n = 1000;
        for (size_t i = 0; i < nops; ++i)
          for (size_t j = i + 1; j < nops; ++j) {
            const std::vector<CastOperand> base = placed(scheme, es, n);
            const std::string msg = fmt("%s and %s overlap", base[i].name, base[j].name);
            const std::string who = std::string(base[i].name) + "/" + base[j].name + w;
            const uintptr_t bi = (uintptr_t)base[i].p, bj = (uintptr_t)base[j].p;
            std::vector<CastOperand> ops = base;
            ops[j].p = reinterpret_cast<const void*>(bi + n * base[i].es - 1);
            expect("last byte shared " + who, wire, wide, scheme, 1, n, ops,
                   BYTEPS_REDUCE_EARGS, msg.c_str());
            ops[j].p = reinterpret_cast<const void*>(bi + n * base[i].es);
            expect("adjacent above " + who, wire, wide, scheme, 1, n, ops, BYTEPS_REDUCE_OK,
                   nullptr);
            ops = base;
            ops[i].p = reinterpret_cast<const void*>(bj + n * base[j].es - 1);
            expect("first byte shared " + who, wire, wide, scheme, 1, n, ops,
                   BYTEPS_REDUCE_EARGS, msg.c_str());
            ops[i].p = reinterpret_cast<const void*>(bj + n * base[j].es);
            expect("adjacent below " + who, wire, wide, scheme, 1, n, ops, BYTEPS_REDUCE_OK,
                   nullptr);
            ops = base;
            ops[j].p = base[i].p;
            expect("same address " + who, wire, wide, scheme, 1, n, ops, BYTEPS_REDUCE_EARGS,
                   msg.c_str());
          }
        // 2^34 elements: stochastic rounding's limit, a count like any other
        // for the rest
        const size_t big = (size_t)1 << 34;
        expect("2^34 elements" + w, wire, wide, scheme, 1, big, placed(scheme, es, big),
               BYTEPS_REDUCE_OK, nullptr);
        expect("2^34 + 1 elements" + w, wire, wide, scheme, 1, big + 1,
               placed(scheme, es, big + 1),
               scheme == kCastSr ? BYTEPS_REDUCE_EARGS : BYTEPS_REDUCE_OK,
               scheme == kCastSr ? "more than 2^34 elements" : nullptr);
      }
    }
  }
  // the overlap of a plain cast reads "dst and src overlap" in both directions
  {
    std::vector<CastOperand> ops = {{"dst", reinterpret_cast<const void*>(0x10000), 4},
                                    {"src", reinterpret_cast<const void*>(0x10004), 2}};
    expect("decompress in place", kBFloat16, kFloat32, kCastPlain, 2, 8, ops,
           BYTEPS_REDUCE_EARGS, "dst and src overlap");
  }
  printf("cases=%d fails=%d\n", g_cases, g_fails);
  return g_fails ? 1 : 0;
}
