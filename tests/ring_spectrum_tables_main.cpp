// Stand-alone host check of the slab tables of a ring's spectrum trace (spectrum_tables::build_slab in
// csrc/bflbm_spectrum.h, included under BFLBM_SPECTRUM_TABLES_ONLY: no HIP, no library).  Built and run by
// tests/test_ring_recorder_abi.py with -fsanitize=address,undefined.
//   usage: ring_spectrum_tables_main nx ny nz nslabs
// For every kind and zero_avg it checks that
//   1. the slabs' lists, mapped back to global half-spectrum indices, partition the half spectrum (minus k = 0 under zero_avg),
//      every entry in the bin the lone build gives it, sorted by (bin, local index);
//   2. no chunk crosses a bin, the chunks tile the list in order, and none is longer than the chunk length or empty;
//   3. the per-bin weighted counts summed over the slabs equal the count of the lone build, and nbins agrees.
// Prints "OK <cases>" and returns 0, or the first failure and 1.
#define BFLBM_SPECTRUM_TABLES_ONLY
#include "bflbm_spectrum.h"

#include <cstdio>
#include <cstdlib>

namespace st = spectrum_tables;

static int failed(const char* what, int kind, int zero_avg, int slab, long long at) {
  std::printf("FAIL %s: kind %d zero_avg %d slab %d at %lld\n", what, kind, zero_avg, slab, at);
  return 1;
}

int main(int argc, char** argv) {
  if (argc != 5) { std::printf("usage: %s nx ny nz nslabs\n", argv[0]); return 2; }
  const int nx = std::atoi(argv[1]), ny = std::atoi(argv[2]), nz = std::atoi(argv[3]), n = std::atoi(argv[4]);
  const int nxc = nx / 2 + 1;
  const long long nk = (long long)nxc * ny * nz;
  int cases = 0;
  for (int kind = 0; kind < 4; ++kind)
    for (int zero_avg = 0; zero_avg < 2; ++zero_avg) {
      const uint64_t L = kind == 0 ? st::shell_lcm(nx, ny, nz) : 1;
      if (!L) return failed("lcm", kind, zero_avg, -1, 0);
      st::Tables lone;
      st::build(nx, ny, nz, kind, zero_avg, L, st::kChunkLen, lone);
      std::vector<int> bin_of((size_t)nk, -1);               // the lone build's bin of every half-spectrum index
      for (const st::Chunk& c : lone.chunks) for (int i = 0; i < c.len; ++i) bin_of[lone.list[(size_t)(c.begin + i)]] = c.bin;
      std::vector<int> seen((size_t)nk, 0);
      std::vector<long long> count((size_t)lone.nbins, 0);
      for (int d = 0; d < n; ++d) {
        const int ky0 = (int)((long long)ny * d / n), ky1 = (int)((long long)ny * (d + 1) / n), nky = ky1 - ky0;
        st::Tables T;
        st::build_slab(nx, ny, nz, ky0, ky1, kind, zero_avg, L, st::kChunkLen, T);
        if (T.nbins != lone.nbins) return failed("nbins", kind, zero_avg, d, T.nbins);
        if ((int)T.bin_first.size() != T.nbins + 1 || T.bin_first[(size_t)T.nbins] != (int)T.chunks.size()) return failed("bin_first", kind, zero_avg, d, 0);
        long long at = 0;
        int most = 0;
        for (size_t ci = 0; ci < T.chunks.size(); ++ci) {
          const st::Chunk& c = T.chunks[ci];
          if (c.begin != at || c.len < 1 || c.len > st::kChunkLen || c.bin < 0 || c.bin >= T.nbins) return failed("chunk shape", kind, zero_avg, d, (long long)ci);
          if ((int)ci < T.bin_first[(size_t)c.bin] || (int)ci >= T.bin_first[(size_t)c.bin + 1]) return failed("chunk outside its bin's range", kind, zero_avg, d, (long long)ci);
          if (ci > 0 && T.chunks[ci - 1].bin > c.bin) return failed("chunk order", kind, zero_avg, d, (long long)ci);
          for (int i = 0; i < c.len; ++i) {
            const uint32_t loc = T.list[(size_t)(c.begin + i)];
            if ((long long)loc >= (long long)nz * nky * nxc) return failed("local index", kind, zero_avg, d, c.begin + i);
            if (i > 0 && T.list[(size_t)(c.begin + i - 1)] >= loc) return failed("index order inside a chunk", kind, zero_avg, d, c.begin + i);
            const int mx = (int)(loc % (uint32_t)nxc), kyl = (int)((loc / (uint32_t)nxc) % (uint32_t)nky), mz = (int)(loc / ((uint32_t)nxc * (uint32_t)nky));
            const long long glob = ((long long)mz * ny + (ky0 + kyl)) * nxc + mx;
            if (bin_of[(size_t)glob] != c.bin) return failed("chunk crosses a bin / wrong bin", kind, zero_avg, d, glob);   // no chunk crosses a bin
            seen[(size_t)glob] += 1;
            count[(size_t)c.bin] += (mx == 0 || 2 * mx == nx) ? 1 : 2;
          }
          if (ci > 0 && T.chunks[ci - 1].bin == c.bin && T.list[(size_t)(c.begin - 1)] >= T.list[(size_t)c.begin]) return failed("index order across chunks", kind, zero_avg, d, (long long)ci);
          at += c.len;
          most = std::max(most, T.bin_first[(size_t)c.bin + 1] - T.bin_first[(size_t)c.bin]);
        }
        if (at != (long long)T.list.size()) return failed("chunks do not tile the list", kind, zero_avg, d, at);
        if (most != T.max_chunks_per_bin) return failed("max_chunks_per_bin", kind, zero_avg, d, most);
      }
      for (long long i = 0; i < nk; ++i)
        if (seen[(size_t)i] != ((zero_avg && i == 0) ? 0 : 1)) return failed("partition of the half spectrum", kind, zero_avg, -1, i);
      for (int s = 0; s < lone.nbins; ++s)
        if (count[(size_t)s] != lone.count[(size_t)s]) return failed("weighted count", kind, zero_avg, -1, s);
      ++cases;
    }
  std::printf("OK %d\n", cases);
  return 0;
}
