// Stand-alone host check of the cluster trace's host part (csrc/bflbm_cluster.h under BFLBM_CLUSTER_HOST_ONLY, on top of
// the host parts of csrc/bflbm_morph.h and csrc/bflbm_fieldsel.h: no HIP, no library).  Built and run by
// tests/test_cluster_abi.py with -fsanitize=address,undefined.  It checks
//   1. every refusal of the arguments, one bad argument each, the message compared in full, and the site limit;
//   2. the geometry: the bricks, the forward directions, the steps on extents 1 and 2, the record's constants, the bins
//      and the packed maximum;
//   3. the algorithm itself: cluster_find and cluster_union, the functions the kernels instantiate, run with a sequential
//      memory policy through the stages of a sample -- the local stage brick by brick, the links that cross a brick face
//      or wrap in forward, reversed and seeded-shuffled order (to imitate arrival orders), flatten, resolve, stats --
//      on small boxes at several fills and both connectivities, labels and record compared with a flood fill of its own
//      that never forms a minimum.
// Every array lives on the heap at its exact length, so an index out of range is the sanitizer's.
// Prints "OK <checks>" and returns 0, or every failure and 1.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <utility>
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
#define BFLBM_MORPH_HOST_ONLY
#include "bflbm_morph.h"
#define BFLBM_CLUSTER_HOST_ONLY
#include "bflbm_cluster.h"

typedef std::vector<double> Doubles;
typedef std::vector<int> Ints;

static int g_checks = 0, g_failed = 0;

static void expect(bool ok, const char* what, const char* detail = "") {
  ++g_checks;
  if (!ok) { ++g_failed; std::printf("FAIL %s %s\n", what, detail); }
}

static void expect_refusal(const char* want, int source, int var, int nlevels, const Doubles* levels, int side, int conn) {
  g_msg.clear();
  const int rc = cluster_refuse_args("X", source, var, nlevels, levels ? levels->data() : nullptr, side, conn);
  expect(rc == 1 && g_msg == want, want, g_msg.c_str());
}

// the sequential stand-in for the kernels' atomics
struct SeqMem {
  int* parent;
  long long* caps;
  int load(int p) const { return parent[p]; }
  int min_old(int p, int v) const { const int old = parent[p]; parent[p] = std::min(old, v); return old; }
  void capped() const { ++*caps; }
};

struct Labelling { Ints labels; std::vector<long long> rec; };

// the stages of a sample with the sequential policy; order 0: the cross-brick links as met, 1: reversed, 2: shuffled
static Labelling pipeline(const ClusterBox& B, const std::vector<char>& occ, int order, unsigned seed, bool* invariant) {
  using namespace cluster_limits;
  const int nsites = B.nx * B.ny * B.nz, ndirs = cluster_ndirs(B.conn);
  Ints parent(nsites, -2), size(nsites, -2);
  long long caps = 0;
  // ---- k_cluster_local, one brick at a time
  const int nbx = (B.nx + kBx - 1) / kBx, nby = (B.ny + kBy - 1) / kBy, nbz = (B.nz + kBz - 1) / kBz;
  for (int bi = 0; bi < nbx * nby * nbz; ++bi) {
    const int x0 = (bi % nbx) * kBx, y0 = ((bi / nbx) % nby) * kBy, z0 = (bi / (nbx * nby)) * kBz;
    Ints sh_parent(kBrick), sh_count(kBrick, 0), site(kBrick, -1);
    SeqMem m{sh_parent.data(), &caps};
    for (int i = 0; i < kBrick; ++i) {
      const int x = x0 + (i & (kBx - 1)), y = y0 + ((i / kBx) & (kBy - 1)), z = z0 + i / (kBx * kBy);
      if (x < B.nx && y < B.ny && z < B.nz) site[i] = (z * B.ny + y) * B.nx + x;
      sh_parent[i] = site[i] >= 0 && occ[site[i]] ? i : -1;
    }
    for (int i = 0; i < kBrick; ++i) {
      if (sh_parent[i] < 0) continue;
      const int p = site[i], z = p / (B.nx * B.ny), y = (p / B.nx) % B.ny, x = p % B.nx;
      for (int d = 0; d < ndirs; ++d) {
        bool local;
        const int q = cluster_neighbour(B, x, y, z, d, &local);
        if (!local) continue;
        const int zq = q / (B.nx * B.ny), yq = (q / B.nx) % B.ny, xq = q % B.nx;
        const int j = ((zq - z0) * kBy + (yq - y0)) * kBx + (xq - x0);
        if (m.load(j) >= 0) cluster_union(m, i, j, kBrick);
      }
    }
    Ints root(kBrick, -1);
    for (int i = 0; i < kBrick; ++i)
      if (sh_parent[i] >= 0) { root[i] = cluster_find(m, i, kBrick); ++sh_count[root[i]]; }
    for (int i = 0; i < kBrick; ++i) {
      if (site[i] < 0) continue;
      parent[site[i]] = root[i] < 0 ? -1 : site[root[i]];
      size[site[i]] = root[i] == i ? sh_count[i] : 0;
    }
  }
  // ---- k_cluster_merge: the links that are not local, in the order asked for
  SeqMem m{parent.data(), &caps};
  std::vector<std::pair<int, int>> links;
  for (int p = 0; p < nsites; ++p) {
    if (parent[p] < 0) continue;
    const int z = p / (B.nx * B.ny), y = (p / B.nx) % B.ny, x = p % B.nx;
    for (int d = 0; d < ndirs; ++d) {
      bool local;
      const int q = cluster_neighbour(B, x, y, z, d, &local);
      if (local || q == p || parent[q] < 0) continue;
      links.push_back(std::make_pair(p, q));
    }
  }
  if (order == 1) std::reverse(links.begin(), links.end());
  if (order == 2) { std::mt19937 gen(seed); std::shuffle(links.begin(), links.end(), gen); }
  for (const auto& l : links) cluster_union(m, m.load(l.first), m.load(l.second), nsites);
  *invariant = true;
  for (int p = 0; p < nsites; ++p) *invariant = *invariant && parent[p] >= -1 && parent[p] <= p && size[p] >= 0;
  // ---- k_cluster_flatten
  Labelling out;
  out.labels.assign(nsites, -1);
  for (int p = 0; p < nsites; ++p)
    if (m.load(p) >= 0) out.labels[p] = cluster_find(m, m.load(p), nsites);
  // ---- k_cluster_resolve
  for (int p = 0; p < nsites; ++p) {
    const int s = size[p];
    if (s <= 0) continue;
    const int r = cluster_find(m, p, nsites);
    if (r == p) continue;
    size[r] += s;
    m.min_old(p, r);
  }
  // ---- k_cluster_stats and k_cluster_finish
  out.rec.assign(kWords, 0);
  unsigned long long best = 0;
  for (int p = 0; p < nsites; ++p) {
    if (parent[p] < 0) continue;
    ++out.rec[1];
    if (parent[p] != p) continue;
    const long long s = size[p];
    ++out.rec[0];
    out.rec[4] += s * s;
    best = std::max(best, cluster_pack((int)s, p));
    ++out.rec[kFirstBin + cluster_bin((int)s)];
  }
  out.rec[2] = cluster_packed_size(best);
  out.rec[3] = cluster_packed_label(best);
  out.rec[kCapped] = caps;
  return out;
}

// the reference of this program: a flood fill over all 6 or 26 offsets, scanned in ascending p, so that the first site
// met of a component is its smallest
static Labelling flood(const ClusterBox& B, const std::vector<char>& occ) {
  const int nsites = B.nx * B.ny * B.nz;
  Labelling out;
  out.labels.assign(nsites, -1);
  out.rec.assign(cluster_limits::kWords, 0);
  out.rec[3] = -1;
  Ints queue;
  for (int p0 = 0; p0 < nsites; ++p0) {
    if (!occ[p0] || out.labels[p0] >= 0) continue;
    queue.assign(1, p0);
    out.labels[p0] = p0;
    for (size_t h = 0; h < queue.size(); ++h) {
      const int p = queue[h], z = p / (B.nx * B.ny), y = (p / B.nx) % B.ny, x = p % B.nx;
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            if (B.conn == 6 && std::abs(dx) + std::abs(dy) + std::abs(dz) != 1) continue;
            const int q = (((z + dz + B.nz) % B.nz) * B.ny + (y + dy + B.ny) % B.ny) * B.nx + (x + dx + B.nx) % B.nx;
            if (occ[q] && out.labels[q] < 0) { out.labels[q] = p0; queue.push_back(q); }
          }
    }
    const long long s = (long long)queue.size();
    ++out.rec[0];
    out.rec[1] += s;
    if (s > out.rec[2]) { out.rec[2] = s; out.rec[3] = p0; }
    out.rec[4] += s * s;
    int b = 0;
    while ((2LL << b) <= s) ++b;
    ++out.rec[6 + b];
  }
  return out;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  using namespace cluster_limits;
  // ---- 1. refusals: one bad argument each -------------------------------------------------------------------------------
  const Doubles good = {0.25, 0.75};
  g_msg.clear();
  expect(cluster_refuse_args("X", 0, 21, 2, good.data(), 1, 6) == 0 && cluster_refuse_args("X", 1, 8, 2, good.data(), 0, 26) == 0 && g_msg.empty(),
         "good arguments pass");
  expect_refusal("X: connectivity must be 6 or 26 (got 18)", 0, 0, 2, &good, 0, 18);
  expect_refusal("X: connectivity must be 6 or 26 (got 0)", 0, 0, 2, &good, 0, 0);
  expect_refusal("X: connectivity must be 6 or 26 (got -6)", 0, 0, 2, &good, 0, -6);
  // the morphology trace's refusals, in its order, before the connectivity
  expect_refusal("X: 1..8 levels (got 0)", 0, 0, 0, &good, 0, 18);
  expect_refusal("X: 1..8 levels (got 9)", 0, 0, 9, &good, 0, 26);
  expect_refusal("X: null argument", 0, 0, 2, nullptr, 0, 26);
  {
    const Doubles l_nan = {0.25, nan}, l_inf = {inf, 0.75};
    expect_refusal("X: level 1 is not finite (got nan)", 0, 0, 2, &l_nan, 0, 26);
    expect_refusal("X: level 0 is not finite (got inf)", 0, 0, 2, &l_inf, 2, 18);
  }
  expect_refusal("X: side must be 0 (v >= level) or 1 (v < level) (got 2)", 0, 0, 2, &good, 2, 18);
  expect_refusal("X: source must be 0 (hydrovs) or 1 (hydrovsbar) (got 2)", 2, 0, 2, &good, 0, 18);
  expect_refusal("X: variable index 22 outside hydrovs (0..21)", 0, 22, 2, &good, 0, 18);
  expect_refusal("X: variable index 9 outside hydrovsbar (0..8)", 1, 9, 2, &good, 0, 26);
  g_msg.clear();
  expect(cluster_refuse_sites("X", 2147483647, 1, 1) == 0 && cluster_refuse_sites("X", 1024, 1024, 1024) == 0 && g_msg.empty(), "2^31 - 1 sites pass");
  expect(cluster_refuse_sites("X", 2048, 2048, 512) == 1 && g_msg == "X: 2147483648 sites exceed 2147483647 (labels are 32-bit)", "the site limit", g_msg.c_str());

  // ---- 2. the geometry and the record's constants -----------------------------------------------------------------------
  expect(kWords == 38 && kBins == 32 && kFirstBin == 6 && kCapped == 5 && kLaunches == 4, "the record");
  expect(kBx == 32 && kBy == 4 && kBz == 4 && kBrick == 512 && kStatsSites == 1024, "the brick");
  expect(cluster_bricks(7, 9, 5) == 6 && cluster_bricks(32, 4, 4) == 1 && cluster_bricks(34, 31, 19) == 80 && cluster_bricks(70, 30, 6) == 48 &&
         cluster_bricks(256, 256, 256) == 32768 && cluster_bricks(1, 1, 1) == 1, "bricks per replica");
  {
    // the forward directions: distinct, lexicographically positive in (dz, dy, dx), and with their negatives all 6 or 26
    bool ok = cluster_ndirs(6) == 3 && cluster_ndirs(26) == 13;
    for (int conn : {6, 26}) {
      const ClusterBox B{5, 5, 5, conn};
      std::vector<char> seen(125, 0);
      for (int k = 0; k < cluster_ndirs(conn); ++k) {
        bool local;
        const int q = cluster_neighbour(B, 2, 2, 2, k, &local);
        const int dz = q / 25 - 2, dy = (q / 5) % 5 - 2, dx = q % 5 - 2;
        ok = ok && local && (dz > 0 || (dz == 0 && (dy > 0 || (dy == 0 && dx > 0)))) && !seen[q];
        if (conn == 6) ok = ok && std::abs(dx) + std::abs(dy) + std::abs(dz) == 1;
        seen[q] = 1;
        seen[((2 - dz) * 5 + 2 - dy) * 5 + 2 - dx] = 1;
      }
      int n = 0;
      for (char s : seen) n += s;
      ok = ok && n == conn;
    }
    expect(ok, "the forward directions");
  }
  {
    int q;
    bool ok = !cluster_step(0, 1, 1, 32, &q) && q == 0 && !cluster_step(0, -1, 1, 4, &q) && q == 0;          // extent 1: its own neighbour
    ok = ok && cluster_step(0, 1, 2, 4, &q) && q == 1 && !cluster_step(0, -1, 2, 4, &q) && q == 1;           // extent 2: + and - coincide
    ok = ok && cluster_step(30, 1, 64, 32, &q) && q == 31 && !cluster_step(31, 1, 64, 32, &q) && q == 32;     // across a brick face
    ok = ok && !cluster_step(31, 1, 32, 32, &q) && q == 0 && !cluster_step(0, -1, 32, 32, &q) && q == 31;     // a brick with itself
    ok = ok && cluster_step(5, 0, 7, 4, &q) && q == 5 && !cluster_step(4, -1, 7, 4, &q) && q == 3;
    expect(ok, "steps: wraps, brick faces, extents 1 and 2");
  }
  expect(cluster_bin(1) == 0 && cluster_bin(2) == 1 && cluster_bin(3) == 1 && cluster_bin(4) == 2 && cluster_bin(1 << 30) == 30 &&
         cluster_bin(2147483647) == 30, "the bins");
  expect(cluster_pack(5, 7) > cluster_pack(5, 9) && cluster_pack(5, 9) > cluster_pack(4, 0) && cluster_packed_size(cluster_pack(5, 7)) == 5 &&
         cluster_packed_label(cluster_pack(5, 7)) == 7 && cluster_packed_label(cluster_pack(2147483647, 2147483646)) == 2147483646 &&
         cluster_packed_size(0) == 0 && cluster_packed_label(0) == -1, "the packed maximum");

  // ---- 3. the algorithm with the sequential policy ------------------------------------------------------------------------
  const int boxes[7][3] = {{7, 9, 5}, {64, 32, 3}, {6, 4, 1}, {2, 2, 2}, {1, 3, 2}, {1, 1, 1}, {33, 17, 6}};
  const double fills[6] = {0.05, 0.1, 0.31, 0.5, 0.8, 1.0};
  for (const auto& n : boxes)
    for (double fill : fills)
      for (int conn : {6, 26}) {
        const ClusterBox B{n[0], n[1], n[2], conn};
        const int nsites = n[0] * n[1] * n[2];
        std::mt19937 gen((unsigned)(1000 * n[0] + 10 * n[1] + n[2] + (int)(100 * fill)));
        std::vector<char> occ(nsites);
        for (char& o : occ) o = (gen() >> 8) * (1.0 / 16777216.0) < fill;
        const Labelling want = flood(B, occ);
        for (int order = 0; order < 3; ++order) {
          bool invariant;
          const Labelling got = pipeline(B, occ, order, 77u + order, &invariant);
          char what[96];
          std::snprintf(what, sizeof what, "box %d x %d x %d fill %.2f connectivity %d order %d", n[0], n[1], n[2], fill, conn, order);
          expect(invariant && got.labels == want.labels && got.rec == want.rec && got.rec[kCapped] == 0, what);
        }
      }

  if (g_failed) return 1;
  std::printf("OK %d\n", g_checks);
  return 0;
}
