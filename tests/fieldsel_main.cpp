// Stand-alone host check of the field-selection layer (the host part of csrc/bflbm_fieldsel.h, included under
// BFLBM_FIELDSEL_HOST_ONLY: no HIP, no library).  Built and run by tests/test_fieldsel_abi.py with
// -fsanitize=address,undefined.  It checks
//   1. the selection of chosen variables for a batch and for a context (mask, nsel, slot, ncomp, vol), the selection of
//      the distinct components of pairs and the pair table, against values written out by hand from the loops the
//      recorders carried before the layer existed;
//   2. every refusal of the variable and pair arguments, one bad argument each, the message compared in full;
//   3. the source helpers.
// The argument arrays live on the heap at their exact length, so a read past nvars or npairs is the sanitizer's.
// Prints "OK <checks>" and returns 0, or every failure and 1.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bflbm.h"
#define BFLBM_NHYDRO_ 22

namespace {
std::string g_msg;
int fail(const char* fmt, ...) {
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  g_msg = buf;
  return 1;
}
}  // namespace

#define BFLBM_FIELDSEL_HOST_ONLY
#include "bflbm_fieldsel.h"

typedef std::vector<int> Ints;

static int g_checks = 0, g_failed = 0;

static void expect(bool ok, const char* what, const char* detail = "") {
  ++g_checks;
  if (!ok) { ++g_failed; std::printf("FAIL %s %s\n", what, detail); }
}

// slots: (component, slot) of the chosen components, every other slot 0; vol: the first entries, the rest 0
static void expect_selection(const char* what, const FieldSelection& f, int source, int nvars, int ncomp, unsigned mask, int nsel,
                             const std::vector<std::pair<int, int>>& slots, const Ints& vol) {
  expect(f.source == source && f.nvars == nvars, what, "source / nvars");
  expect(f.ncomp == ncomp, what, "ncomp");
  expect(f.sel.mask == mask, what, "mask");
  expect(f.sel.nsel == nsel, what, "nsel");
  int want_slot[BFLBM_NHYDRO_] = {};
  for (const auto& s : slots) want_slot[s.first] = s.second;
  expect(std::memcmp(f.sel.slot, want_slot, sizeof want_slot) == 0, what, "slot");
  int want_vol[fstat_limits::kMaxVars] = {};
  for (size_t i = 0; i < vol.size(); ++i) want_vol[i] = vol[i];
  expect(std::memcmp(f.vol.vol, want_vol, sizeof want_vol) == 0, what, "vol");
}

static void expect_both(const char* what, int source, const Ints& vars, int ncomp, unsigned mask,
                        const std::vector<std::pair<int, int>>& slots, const Ints& batch_vol) {
  const int n = (int)vars.size();
  expect_selection(what, field_select(true, source, n, vars.data()), source, n, ncomp, mask, (int)slots.size(), slots, batch_vol);
  expect_selection(what, field_select(false, source, n, vars.data()), source, n, ncomp, 0u, 0, {}, vars);   // a context reads components
}

static void expect_refusal(const char* want, int source, int max_source, const Ints& vars, int nvars, int npairs, const Ints* a, const Ints* b) {
  g_msg.clear();
  const int rc = field_refuse_args("X", source, max_source, nvars, vars.data(), npairs, a ? a->data() : nullptr, b ? b->data() : nullptr);
  expect(rc == 1 && g_msg == want, want, g_msg.c_str());
}

int main() {
  // ---- 1. selections ---------------------------------------------------------------------------------------------------
  // hydrovs 3, 1, 21: ascending 1, 3, 21 take the slots 0, 1, 2; bits 1, 3, 21
  expect_both("hydrovs {3, 1, 21}", 0, {3, 1, 21}, 22, 2u + 8u + 2097152u, {{1, 0}, {3, 1}, {21, 2}}, {1, 0, 2});
  expect_both("hydrovs {0}", 0, {0}, 1, 1u, {{0, 0}}, {0});
  // eight: ascending 0, 2, 4, 5, 7, 9, 12, 20
  expect_both("hydrovs, eight variables", 0, {7, 0, 5, 2, 20, 9, 12, 4}, 21, 1u + 4u + 16u + 32u + 128u + 512u + 4096u + 1048576u,
              {{0, 0}, {2, 1}, {4, 2}, {5, 3}, {7, 4}, {9, 5}, {12, 6}, {20, 7}}, {4, 0, 3, 1, 7, 5, 6, 2});
  // hydrovsbar: a context's observation produces all nine components whatever is chosen
  expect_both("hydrovsbar {8, 2}", 1, {8, 2}, 9, 256u + 4u, {{2, 0}, {8, 1}}, {1, 0});
  // the noise moments: contexts only (a batch has no noise form and is refused before the selection)
  {
    const Ints vars = {37, 0, 19};
    expect_selection("noise {37, 0, 19}", field_select(false, 2, 3, vars.data()), 2, 3, 38, 0u, 0, {}, vars);
  }
  // the distinct components of pairs, for a context too: (5, 0), (0, 0), (5, 17) choose 0, 5, 17
  {
    const Ints a = {5, 0, 5}, b = {0, 0, 17};
    expect_selection("pairs of hydrovs", field_select_pairs(0, 3, a.data(), b.data()), 0, 3, 18, 1u + 32u + 131072u, 3,
                     {{0, 0}, {5, 1}, {17, 2}}, {0, 1, 2});
    const Ints c = {8}, d = {8};
    expect_selection("a pair of hydrovsbar", field_select_pairs(1, 1, c.data(), d.data()), 1, 1, 9, 256u, 1, {{8, 0}}, {0});
  }
  {
    const Ints a = {0, 2, 1}, b = {0, 1, 1};
    const FstatPairs P = field_pairs(3, a.data(), b.data());
    int wa[fstat_limits::kMaxPairs] = {0, 2, 1}, wb[fstat_limits::kMaxPairs] = {0, 1, 1}, zero[fstat_limits::kMaxPairs] = {};
    expect(P.n == 3 && std::memcmp(P.a, wa, sizeof wa) == 0 && std::memcmp(P.b, wb, sizeof wb) == 0, "pair table of three");
    const FstatPairs N = field_pairs(0, nullptr, nullptr);
    expect(N.n == 0 && std::memcmp(N.a, zero, sizeof zero) == 0 && std::memcmp(N.b, zero, sizeof zero) == 0, "empty pair table");
  }

  // ---- 2. refusals: one bad argument each ------------------------------------------------------------------------------
  const Ints good = {3, 1}, pa = {0, 1}, pb = {1, 1};
  g_msg.clear();
  expect(field_refuse_args("X", 0, 1, 2, good.data(), 2, pa.data(), pb.data()) == 0 && g_msg.empty(), "good arguments pass");
  expect(field_refuse_args("X", 2, 2, 2, good.data(), 0, nullptr, nullptr) == 0 && g_msg.empty(), "good noise arguments pass");
  expect_refusal("X: source must be 0 (hydrovs) or 1 (hydrovsbar) (got -1)", -1, 1, good, 2, 0, nullptr, nullptr);
  expect_refusal("X: source must be 0 (hydrovs) or 1 (hydrovsbar) (got 2)", 2, 1, good, 2, 0, nullptr, nullptr);
  expect_refusal("X: source must be 0 (hydrovs), 1 (hydrovsbar) or 2 (noise) (got 3)", 3, 2, good, 2, 0, nullptr, nullptr);
  expect_refusal("X: 1..8 variables (got 0)", 0, 1, Ints(), 0, 0, nullptr, nullptr);
  expect_refusal("X: 1..8 variables (got 9)", 0, 1, {0, 1, 2, 3, 4, 5, 6, 7, 8}, 9, 0, nullptr, nullptr);
  expect_refusal("X: 0..16 pairs (got 17)", 0, 1, good, 2, 17, &pa, &pb);
  expect_refusal("X: 0..16 pairs (got -1)", 0, 1, good, 2, -1, &pa, &pb);
  expect_refusal("X: null argument", 0, 1, good, 2, 2, nullptr, &pb);
  expect_refusal("X: null argument", 0, 1, good, 2, 2, &pa, nullptr);
  expect_refusal("X: variable index 22 outside hydrovs (0..21)", 0, 1, {3, 22}, 2, 0, nullptr, nullptr);
  expect_refusal("X: variable index -1 outside hydrovs (0..21)", 0, 2, {-1, 3}, 2, 0, nullptr, nullptr);
  expect_refusal("X: variable index 9 outside hydrovsbar (0..8)", 1, 1, {9}, 1, 0, nullptr, nullptr);
  expect_refusal("X: variable index 38 outside the noise moments (0..37)", 2, 2, {37, 38}, 2, 0, nullptr, nullptr);
  expect_refusal("X: variable index 3 given twice", 0, 1, {3, 1, 3}, 3, 0, nullptr, nullptr);
  {
    const Ints a = {0, 2}, b = {1, 0}, c = {0}, d = {-1};
    expect_refusal("X: pair 1: slot 2 outside the 2 variables", 0, 1, good, 2, 2, &a, &b);
    expect_refusal("X: pair 0: slot -1 outside the 2 variables", 1, 1, good, 2, 1, &c, &d);
  }
  {
    const Ints a = {0, 5}, b = {1, 22}, c = {9}, d = {0};
    g_msg.clear();
    expect(field_refuse_pair_vars("X", 0, 2, a.data(), b.data()) == 1 && g_msg == "X: pair 1: variable index 22 outside hydrovs (0..21)", "pair variables of hydrovs", g_msg.c_str());
    expect(field_refuse_pair_vars("X", 1, 1, c.data(), d.data()) == 1 && g_msg == "X: pair 0: variable index 9 outside hydrovsbar (0..8)", "pair variables of hydrovsbar", g_msg.c_str());
    g_msg.clear();
    expect(field_refuse_pair_vars("X", 0, 2, a.data(), a.data()) == 0 && g_msg.empty(), "good pair variables pass");
  }

  // ---- 3. the sources --------------------------------------------------------------------------------------------------
  expect(field_source_size(0) == 22 && field_source_size(1) == 9 && field_source_size(2) == 38, "source sizes");
  expect(field_observe_code(0) == 2 && field_observe_code(1) == 0 && field_observe_code(2) == 1, "observation codes");
  expect(std::string(field_source_name(0)) == "hydrovs" && std::string(field_source_name(1)) == "hydrovsbar" &&
         std::string(field_source_name(2)) == "the noise moments", "source names");
  const ObsSel first = obs_first(3);
  expect(first.mask == 7u && first.nsel == 3 && first.slot[2] == 2 && first.slot[3] == 0, "obs_first");

  if (g_failed) return 1;
  std::printf("OK %d\n", g_checks);
  return 0;
}
