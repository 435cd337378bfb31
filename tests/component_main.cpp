// Stand-alone host check of the component trace's host part (csrc/bflbm_components.h under BFLBM_COMPONENTS_HOST_ONLY, on
// top of the host parts of csrc/bflbm_cluster.h, csrc/bflbm_morph.h and csrc/bflbm_fieldsel.h: no HIP, no library).  Built
// and run by tests/test_component_abi.py with -fsanitize=address,undefined; never loaded into another process.  It checks
//   1. every refusal of the arguments, one bad argument each, the message compared in full, and the extent limit;
//   2. the layout's constants, component_offset, component_wrap and component_key;
//   3. component_arc against a brute-force circular scan on random arcs, full and empty axes, across word boundaries;
//   4. the stages of a sample with sequential stand-ins for the atomics -- the cluster trace's labelling through
//      cluster_find and cluster_union, then count, scan and rank in groups of kRankSites, the masks brick by brick with the
//      key and flush rule of k_component_masks, component_arc, the moments brick by brick keyed and flushed as
//      k_component_moments does, finish -- on small random boxes at several fills, both connectivities and the three
//      (min_size, rows) pairs, header and rows compared with a brute force over a flood fill of its own.
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
#define BFLBM_COMPONENTS_HOST_ONLY
#include "bflbm_components.h"

typedef std::vector<double> Doubles;
typedef std::vector<int> Ints;
typedef std::vector<long long> Words;
typedef unsigned long long u64;

static int g_checks = 0, g_failed = 0;

static void expect(bool ok, const char* what, const char* detail = "") {
  ++g_checks;
  if (!ok) { ++g_failed; std::printf("FAIL %s %s\n", what, detail); }
}

static void expect_refusal(const char* want, int nlevels, const Doubles* levels, int conn, long long min_size, int rows) {
  g_msg.clear();
  const int rc = component_refuse_args("X", 0, 0, nlevels, levels ? levels->data() : nullptr, 0, conn, min_size, rows);
  expect(rc == 1 && g_msg == want, want, g_msg.c_str());
}

struct SeqMem {
  int* parent;
  long long* caps;
  int load(int p) const { return parent[p]; }
  int min_old(int p, int v) const { const int old = parent[p]; parent[p] = std::min(old, v); return old; }
  void capped() const { ++*caps; }
};

struct Brick { int x0, y0, z0; Ints site; };   // site[i]: the linear index of brick-local i, -1 outside the box

static std::vector<Brick> bricks_of(const ClusterBox& B) {
  using namespace cluster_limits;
  const int nbx = (B.nx + kBx - 1) / kBx, nby = (B.ny + kBy - 1) / kBy, nbz = (B.nz + kBz - 1) / kBz;
  std::vector<Brick> out;
  for (int bi = 0; bi < nbx * nby * nbz; ++bi) {
    Brick b{(bi % nbx) * kBx, ((bi / nbx) % nby) * kBy, (bi / (nbx * nby)) * kBz, Ints(kBrick, -1)};
    for (int i = 0; i < kBrick; ++i) {
      const int x = b.x0 + (i & (kBx - 1)), y = b.y0 + ((i / kBx) & (kBy - 1)), z = b.z0 + i / (kBx * kBy);
      if (x < B.nx && y < B.ny && z < B.nz) b.site[i] = (z * B.ny + y) * B.nx + x;
    }
    out.push_back(b);
  }
  return out;
}

// local, merge and resolve of the cluster trace with the sequential policy; the cross-brick links reversed when asked
static void label(const ClusterBox& B, const std::vector<char>& occ, bool reversed, Ints& parent, Ints& size, long long* caps) {
  using namespace cluster_limits;
  const int nsites = B.nx * B.ny * B.nz, ndirs = cluster_ndirs(B.conn);
  parent.assign(nsites, -2); size.assign(nsites, -2);
  for (const Brick& b : bricks_of(B)) {
    Ints sh_parent(kBrick), sh_count(kBrick, 0), root(kBrick, -1);
    SeqMem m{sh_parent.data(), caps};
    for (int i = 0; i < kBrick; ++i) sh_parent[i] = b.site[i] >= 0 && occ[b.site[i]] ? i : -1;
    for (int i = 0; i < kBrick; ++i) {
      if (sh_parent[i] < 0) continue;
      const int p = b.site[i], z = p / (B.nx * B.ny), y = (p / B.nx) % B.ny, x = p % B.nx;
      for (int d = 0; d < ndirs; ++d) {
        bool local;
        const int q = cluster_neighbour(B, x, y, z, d, &local);
        if (!local) continue;
        const int j = component_key(B, b.x0, b.y0, b.z0, q);
        if (m.load(j) >= 0) cluster_union(m, i, j, kBrick);
      }
    }
    for (int i = 0; i < kBrick; ++i)
      if (sh_parent[i] >= 0) { root[i] = cluster_find(m, i, kBrick); ++sh_count[root[i]]; }
    for (int i = 0; i < kBrick; ++i) {
      if (b.site[i] < 0) continue;
      parent[b.site[i]] = root[i] < 0 ? -1 : b.site[root[i]];
      size[b.site[i]] = root[i] == i ? sh_count[i] : 0;
    }
  }
  SeqMem m{parent.data(), caps};
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
  if (reversed) std::reverse(links.begin(), links.end());
  for (const auto& l : links) cluster_union(m, m.load(l.first), m.load(l.second), nsites);
  for (int p = 0; p < nsites; ++p) {
    const int s = size[p];
    if (s <= 0) continue;
    const int r = cluster_find(m, p, nsites);
    if (r == p) continue;
    size[r] += s;
    m.min_old(p, r);
  }
}

// key and slot of an occupied in-range site, as component_site in the kernels' header
static bool site_key(const ClusterBox& B, const Brick& b, int i, const Ints& parent, const Ints& size, int rows, int* key, int* slot) {
  const int up = parent[b.site[i]];
  if (up < 0) return false;
  const int k = component_key(B, b.x0, b.y0, b.z0, up);
  *slot = size[parent[up]];
  if (*slot < 0 || *slot >= rows) return false;
  *key = k < 0 ? i : k;
  return true;
}

// the stages after the labelling: one level's record, 6 + rows 18 words
static Words sample(const ClusterBox& B, Ints parent, Ints size, long long min_size, int rows, long long caps, long long* flushes) {
  using namespace cluster_limits;
  using namespace component_limits;
  const int nsites = B.nx * B.ny * B.nz;
  std::vector<u64> stage(component_words(rows), 0);
  u64* row0 = stage.data() + kHeader;
  stage[component_limits::kCapped] = (u64)caps;
  // ---- count, scan, rank
  const int groups = (int)component_groups(nsites);
  std::vector<unsigned> counts(groups, 0);
  for (int g = 0; g < groups; ++g)
    for (int p = g * kRankSites; p < std::min(nsites, (g + 1) * kRankSites); ++p) {
      if (parent[p] < 0) continue;
      ++stage[1];
      if (parent[p] != p) continue;
      ++stage[0];
      if (size[p] >= min_size) { ++stage[2]; stage[3] += size[p]; ++counts[g]; }
    }
  unsigned carry = 0;
  for (int g = 0; g < groups; ++g) { const unsigned v = counts[g]; counts[g] = carry; carry += v; }
  for (int g = groups - 1; g >= 0; --g) {                  // the groups in any order: the rank does not depend on it
    unsigned rank = counts[g];
    for (int p = g * kRankSites; p < std::min(nsites, (g + 1) * kRankSites); ++p) {
      if (parent[p] != p) continue;
      int slot = -1;
      if (size[p] >= min_size) {
        if (rank < (unsigned)rows) { slot = (int)rank; row0[slot * kRowWords + kLabel] = p; row0[slot * kRowWords + kSize] = size[p]; }
        ++rank;
      }
      size[p] = slot;
    }
  }
  // ---- masks, brick by brick: LDS words per key, one flush per (key present, axis)
  const int wx = component_mask_words(B.nx), wy = component_mask_words(B.ny), sw = component_slot_words(B);
  std::vector<u64> masks((size_t)rows * sw, 0);
  const std::vector<Brick> bricks = bricks_of(B);
  for (const Brick& b : bricks) {
    std::vector<unsigned> sh_x(kBrick, 0), sh_yz(kBrick, 0);
    Ints sh_slot(kBrick, -1);
    for (int i = 0; i < kBrick; ++i) {
      int key, slot;
      if (b.site[i] < 0 || !site_key(B, b, i, parent, size, rows, &key, &slot)) continue;
      sh_x[key] |= 1u << (i & (kBx - 1));
      sh_yz[key] |= (1u << ((i / kBx) & (kBy - 1))) | (16u << (i / (kBx * kBy)));
      sh_slot[key] = slot;
    }
    for (int i = 0; i < kBrick; ++i) {
      if (sh_slot[i] < 0) continue;
      u64* m = masks.data() + (size_t)sh_slot[i] * sw;
      m[b.x0 >> 6] |= (u64)sh_x[i] << (b.x0 & 63);
      m[wx + (b.y0 >> 6)] |= (u64)(sh_yz[i] & 15u) << (b.y0 & 63);
      m[wx + wy + (b.z0 >> 6)] |= (u64)(sh_yz[i] >> 4) << (b.z0 & 63);
      *flushes += 3;
    }
  }
  // ---- origin
  for (int slot = 0; slot < rows; ++slot)
    for (int axis = 0; axis < 3; ++axis) {
      const int n = axis == 0 ? B.nx : (axis == 1 ? B.ny : B.nz);
      long long origin, extent;
      component_arc(masks.data() + (size_t)slot * sw + (axis == 0 ? 0 : (axis == 1 ? wx : wx + wy)), n, &origin, &extent);
      row0[slot * kRowWords + kOrigin + axis] = (u64)origin;
      row0[slot * kRowWords + kExtent + axis] = (u64)extent;
    }
  // ---- moments, brick by brick
  for (const Brick& b : bricks) {
    std::vector<u64> sh_sum((size_t)kSums * kBrick, 0);
    Ints sh_slot(kBrick, -1);
    for (int i = 0; i < kBrick; ++i) {
      int key, slot;
      if (b.site[i] < 0 || !site_key(B, b, i, parent, size, rows, &key, &slot)) continue;
      const int p = b.site[i], z = p / (B.nx * B.ny), y = (p / B.nx) % B.ny, x = p % B.nx;
      const u64* row = row0 + slot * kRowWords;
      const u64 dx = component_offset(x, (int)row[kOrigin], B.nx), dy = component_offset(y, (int)row[kOrigin + 1], B.ny),
                dz = component_offset(z, (int)row[kOrigin + 2], B.nz);
      u64 faces = 0;
      for (int d = -1; d <= 1; d += 2) {
        faces += parent[(z * B.ny + y) * B.nx + component_wrap(x, d, B.nx)] < 0;
        faces += parent[(z * B.ny + component_wrap(y, d, B.ny)) * B.nx + x] < 0;
        faces += parent[(component_wrap(z, d, B.nz) * B.ny + y) * B.nx + x] < 0;
      }
      const u64 v[kSums] = {dx, dy, dz, dx * dx, dy * dy, dz * dz, dx * dy, dx * dz, dy * dz, faces};
      for (int j = 0; j < kSums; ++j) sh_sum[(size_t)j * kBrick + key] += v[j];
      sh_slot[key] = slot;
    }
    for (int i = 0; i < kBrick; ++i) {
      if (sh_slot[i] < 0) continue;
      for (int j = 0; j < kSums; ++j) row0[sh_slot[i] * kRowWords + kSum + j] += sh_sum[(size_t)j * kBrick + i];
    }
  }
  // ---- finish
  Words out(stage.size());
  for (size_t w = 0; w < stage.size(); ++w) out[w] = (long long)stage[w];
  out[4] = std::min<long long>(out[2], rows);
  for (int slot = 0; slot < rows; ++slot)
    if (stage[kHeader + slot * kRowWords + kSize] == 0) {
      for (int w = 0; w < kRowWords; ++w) out[kHeader + slot * kRowWords + w] = 0;
      out[kHeader + slot * kRowWords + kLabel] = -1;
    }
  return out;
}

// the reference of this program: a flood fill scanned in ascending p, per component explicit site lists, the arc by a
// circular scan, sums by loops
static Words brute(const ClusterBox& B, const std::vector<char>& occ, long long min_size, int rows, bool* single_arc) {
  const int nsites = B.nx * B.ny * B.nz, n[3] = {B.nx, B.ny, B.nz};
  Words out(component_words(rows), 0);
  for (int slot = 0; slot < rows; ++slot) out[6 + slot * 18] = -1;
  Ints labels(nsites, -1), queue;
  int used = 0;
  for (int p0 = 0; p0 < nsites; ++p0) {
    if (!occ[p0] || labels[p0] >= 0) continue;
    queue.assign(1, p0);
    labels[p0] = p0;
    for (size_t h = 0; h < queue.size(); ++h) {
      const int p = queue[h], z = p / (B.nx * B.ny), y = (p / B.nx) % B.ny, x = p % B.nx;
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            if (B.conn == 6 && std::abs(dx) + std::abs(dy) + std::abs(dz) != 1) continue;
            const int q = (((z + dz + B.nz) % B.nz) * B.ny + (y + dy + B.ny) % B.ny) * B.nx + (x + dx + B.nx) % B.nx;
            if (occ[q] && labels[q] < 0) { labels[q] = p0; queue.push_back(q); }
          }
    }
    const long long s = (long long)queue.size();
    ++out[0]; out[1] += s;
    int origin[3], extent[3];
    for (int a = 0; a < 3; ++a) {
      std::vector<char> present(n[a], 0);
      for (int p : queue) present[a == 0 ? p % B.nx : (a == 1 ? (p / B.nx) % B.ny : p / (B.nx * B.ny))] = 1;
      int starts = 0;
      origin[a] = 0; extent[a] = 0;
      for (int c = n[a] - 1; c >= 0; --c) {
        extent[a] += present[c];
        if (present[c] && !present[(c + n[a] - 1) % n[a]]) { origin[a] = c; ++starts; }
      }
      *single_arc = *single_arc && (starts == 1 || (starts == 0 && extent[a] == n[a]));
    }
    if (s < min_size) continue;
    ++out[2]; out[3] += s;
    if (used == rows) continue;
    long long* row = out.data() + 6 + used * 18;
    row[0] = p0; row[1] = s;
    for (int a = 0; a < 3; ++a) { row[2 + a] = origin[a]; row[5 + a] = extent[a]; }
    for (int p : queue) {
      const int c[3] = {p % B.nx, (p / B.nx) % B.ny, p / (B.nx * B.ny)};
      long long d[3];
      for (int a = 0; a < 3; ++a) { d[a] = (c[a] - origin[a] + n[a]) % n[a]; row[8 + a] += d[a]; row[11 + a] += d[a] * d[a]; }
      row[14] += d[0] * d[1]; row[15] += d[0] * d[2]; row[16] += d[1] * d[2];
      for (int a = 0; a < 3; ++a)
        for (int dir = -1; dir <= 1; dir += 2) {
          int q[3] = {c[0], c[1], c[2]};
          q[a] = (q[a] + dir + n[a]) % n[a];
          row[17] += !occ[(q[2] * B.ny + q[1]) * B.nx + q[0]];
        }
    }
    ++used;
  }
  out[4] = used;
  return out;
}

int main() {
  using namespace component_limits;
  // ---- 1. refusals: one bad argument each -------------------------------------------------------------------------------
  const Doubles good = {0.25, 0.75};
  g_msg.clear();
  expect(component_refuse_args("X", 0, 21, 2, good.data(), 1, 6, 1, 1) == 0 && component_refuse_args("X", 1, 8, 2, good.data(), 0, 26, 1LL << 40, 256) == 0 &&
         g_msg.empty(), "good arguments pass");
  expect_refusal("X: min_size must be >= 1 (got 0)", 2, &good, 26, 0, 4);
  expect_refusal("X: min_size must be >= 1 (got -5)", 2, &good, 6, -5, 0);
  expect_refusal("X: rows must be in 1..256 (got 0)", 2, &good, 26, 1, 0);
  expect_refusal("X: rows must be in 1..256 (got 257)", 2, &good, 26, 1, 257);
  expect_refusal("X: rows must be in 1..256 (got -1)", 2, &good, 26, 1, -1);
  // the cluster trace's refusals come first
  expect_refusal("X: connectivity must be 6 or 26 (got 18)", 2, &good, 18, 0, 0);
  expect_refusal("X: 1..8 levels (got 9)", 9, &good, 18, 0, 0);
  expect_refusal("X: null argument", 2, nullptr, 26, 1, 4);
  g_msg.clear();
  expect(component_refuse_sites("X", 65536, 4, 4) == 0 && component_refuse_sites("X", 1, 1, 65536) == 0 && g_msg.empty(), "an extent of 65536 passes");
  expect(component_refuse_sites("X", 65537, 1, 1) == 1 && g_msg == "X: an extent of 65537 exceeds 65536 (the second moments are 64-bit)", "the extent limit",
         g_msg.c_str());
  expect(component_refuse_sites("X", 2048, 2048, 512) == 1 && g_msg == "X: 2147483648 sites exceed 2147483647 (labels are 32-bit)", "the site limit",
         g_msg.c_str());

  // ---- 2. the layout ------------------------------------------------------------------------------------------------------
  expect(kHeader == 6 && kRowWords == 18 && kMaxRows == 256 && kLaunches == 9 && kSums == 10 && kRankSites == 1024 && kCapped == cluster_limits::kCapped,
         "the record");
  expect(kLabel == 0 && kSize == 1 && kOrigin == 2 && kExtent == 5 && kSum == 8 && kSum2 == 11 && kCross == 14 && kFaces == 17, "the row");
  expect(component_words(256) == 4614 && component_words(1) == 24 && component_mask_words(1) == 1 && component_mask_words(64) == 1 &&
         component_mask_words(65) == 2 && component_slot_words(ClusterBox{70, 30, 6, 26}) == 4 && component_groups(1025) == 2, "words and groups");
  expect(component_offset(3, 3, 7) == 0 && component_offset(2, 5, 7) == 4 && component_offset(6, 0, 7) == 6 && component_wrap(0, -1, 5) == 4 &&
         component_wrap(4, 1, 5) == 0 && component_wrap(0, 1, 1) == 0 && component_wrap(0, -1, 1) == 0 && component_wrap(1, 1, 2) == 0 &&
         component_wrap(1, -1, 2) == 0, "offsets and wraps");
  {
    const ClusterBox B{70, 30, 6, 26};
    bool ok = component_key(B, 32, 4, 4, (4 * 30 + 4) * 70 + 32) == 0 && component_key(B, 32, 4, 4, (5 * 30 + 7) * 70 + 63) == (1 * 4 + 3) * 32 + 31;
    ok = ok && component_key(B, 32, 4, 4, (4 * 30 + 4) * 70 + 31) == -1 && component_key(B, 32, 4, 4, (4 * 30 + 8) * 70 + 32) == -1 &&
         component_key(B, 32, 4, 4, (3 * 30 + 4) * 70 + 32) == -1 && component_key(B, 32, 4, 4, (4 * 30 + 4) * 70 + 64) == -1;
    expect(ok, "the key: inside and just outside the brick");
  }

  // ---- 3. the arc function against a circular scan ----------------------------------------------------------------------------
  {
    std::mt19937 gen(9);
    bool ok = true;
    for (int n : {1, 2, 3, 7, 63, 64, 65, 127, 128, 129, 200}) {
      for (int trial = 0; trial < 40 && ok; ++trial) {
        const int start = (int)(gen() % n), length = trial == 0 ? 0 : (trial == 1 ? n : 1 + (int)(gen() % n));
        std::vector<u64> w(component_mask_words(n), 0);
        std::vector<char> present(n, 0);
        for (int k = 0; k < length; ++k) { const int c = (start + k) % n; present[c] = 1; w[c >> 6] |= 1ull << (c & 63); }
        long long want_origin = 0, want_extent = 0, origin = -7, extent = -7;
        for (int c = n - 1; c >= 0; --c) { want_extent += present[c]; if (present[c] && !present[(c + n - 1) % n]) want_origin = c; }
        component_arc(w.data(), n, &origin, &extent);
        ok = origin == want_origin && extent == want_extent && (length == 0 || length == n ? origin == 0 : origin == start);
        if (!ok) std::printf("arc n %d start %d length %d: origin %lld extent %lld\n", n, start, length, origin, extent);
      }
    }
    expect(ok, "component_arc on arcs, full and empty axes");
  }

  // ---- 4. the stages with the sequential policy -----------------------------------------------------------------------------
  const int boxes[7][3] = {{7, 9, 5}, {64, 32, 3}, {6, 4, 1}, {2, 2, 2}, {1, 3, 2}, {70, 9, 6}, {33, 17, 6}};
  const double fills[6] = {0.05, 0.1, 0.31, 0.5, 0.8, 1.0};
  const long long pairs[3][2] = {{1, 256}, {1, 4}, {3, 16}};
  bool overflowed = false, fitted = false, single_arc = true, shared_key = false;
  for (const auto& n : boxes)
    for (double fill : fills)
      for (int conn : {6, 26}) {
        const ClusterBox B{n[0], n[1], n[2], conn};
        const int nsites = n[0] * n[1] * n[2];
        std::mt19937 gen((unsigned)(1000 * n[0] + 10 * n[1] + n[2] + (int)(100 * fill)));
        std::vector<char> occ(nsites);
        for (char& o : occ) o = (gen() >> 8) * (1.0 / 16777216.0) < fill;
        for (int order = 0; order < 2; ++order) {
          Ints parent, size;
          long long caps = 0;
          label(B, occ, order == 1, parent, size, &caps);
          for (const auto& pr : pairs) {
            long long flushes = 0;
            const Words got = sample(B, parent, size, pr[0], (int)pr[1], caps, &flushes);
            const Words want = brute(B, occ, pr[0], (int)pr[1], &single_arc);
            char what[112];
            std::snprintf(what, sizeof what, "box %d x %d x %d fill %.2f connectivity %d order %d min_size %lld rows %lld", n[0], n[1], n[2], fill, conn,
                          order, pr[0], pr[1]);
            expect(got == want && got[kCapped] == 0, what);
            overflowed = overflowed || want[2] > pr[1];
            fitted = fitted || (want[2] > 0 && want[2] <= pr[1]);
            // the flush rule: at most one flush per (site of a tabulated component) and far fewer where components are large
            long long tabulated = 0;
            for (int slot = 0; slot < pr[1]; ++slot) tabulated += want[6 + slot * 18 + 1];
            shared_key = shared_key || (flushes > 0 && flushes < 3 * tabulated / 8);
            if (flushes > 3 * tabulated) expect(false, what, "more flushes than sites");
          }
        }
      }
  expect(overflowed && fitted, "the inputs overflow the rows and fit them");
  expect(single_arc, "every projection is one arc");
  expect(shared_key, "the sites of a brick share a key");

  if (g_failed) return 1;
  std::printf("OK %d\n", g_checks);
  return 0;
}
