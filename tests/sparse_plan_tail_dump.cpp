// Stand-alone program (sparse_plan.cpp + knobs.cpp, no GPU, no libsfb.so): prints the forward sweep schedule of every pattern of a
// zoo file (the format tests/sparse_zoo.py writes and tests/sparse_plan_check.cpp reads) as one JSON line per plan,
//   {"name", "k", "nnzL", "funits", "ftail0", "ftail", "idx_scale", "counts": [slots of unit u],
//    "tail": [[ [row, column, lane, half] of every slot of unit ftail0 + i ] for i < ftail], "lcols": [entries of L in column j, j >= k - 1 - ftail]}
// for tests/test_sparse_plan_tail_host.py.  The schedule itself is verified by sparse_plan_check.cpp; this only shows the layout.
#include "../smooth_feedback_amd/csrc/sparse_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using sfb::SparsePlanHost;

namespace {
struct Reader {
  FILE *f;
  void raw(void *p, size_t bytes)
  {
    if (bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "zoo file: short read\n"); exit(2); }
  }
  int32_t i32() { int32_t v; raw(&v, 4); return v; }
  std::vector<int32_t> ints(size_t c)
  {
    if (c > (1u << 26)) { fprintf(stderr, "zoo file: bad count\n"); exit(2); }
    std::vector<int32_t> v(c);
    raw(v.data(), 4 * c);
    return v;
  }
  void skip_doubles(size_t c)
  {
    std::vector<double> v(c);
    raw(v.data(), 8 * c);
  }
};
}  // namespace

int main(int argc, char **argv)
{
  if (argc != 2) { fprintf(stderr, "usage: %s ZOOFILE\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  Reader r{f};
  char magic[8];
  r.raw(magic, 8);
  if (memcmp(magic, "SFBZOO1", 8) != 0) { fprintf(stderr, "zoo file: bad magic\n"); return 2; }
  const int count = r.i32();
  SparsePlanHost prev;
  for (int e = 0; e < count; ++e) {
    const int len = r.i32();
    if (len < 1 || len > 200) { fprintf(stderr, "zoo file: bad name\n"); return 2; }
    std::string name((size_t)len, ' ');
    r.raw(&name[0], (size_t)len);
    const std::vector<int32_t> h = r.ints(8);
    const int n = h[0], m = h[1], k = n + m;
    if (n < 1 || m < 1 || h[6] < 0 || h[7] < 0) { fprintf(stderr, "zoo file: bad sizes\n"); return 2; }
    const std::vector<int32_t> Pp = r.ints((size_t)n + 1), Pi = r.ints((size_t)h[6]), Ap = r.ints((size_t)m + 1), Aj = r.ints((size_t)h[7]);
    std::vector<int32_t> perm, stage;
    if (h[3]) perm = r.ints((size_t)k);
    if (h[4]) stage = r.ints((size_t)k);
    r.skip_doubles((size_t)h[6] + (size_t)h[7] + 2 * (size_t)k);
    const bool chain = h[5] != 0;  // the whole-pattern fallback of the entry before it: that plan's perm and LDS
    if (chain && prev.k != k) { fprintf(stderr, "%s: chained entry without a predecessor\n", name.c_str()); return 2; }
    SparsePlanHost pl;
    const char *msg = "";
    const int32_t *up = chain ? prev.perm.data() : (h[3] ? perm.data() : nullptr);
    if (!sfb::build_sparse_plan(n, m, Pp.data(), Pi.data(), Ap.data(), Aj.data(), h[2], up, h[4] && !chain ? stage.data() : nullptr, pl,
                                &msg, chain ? prev.lds_doubles : 0)) {
      fprintf(stderr, "%s: refused: %s\n", name.c_str(), msg);
      return 1;
    }
    const int sc = pl.idx_scale;
    printf("{\"name\": \"%s\", \"k\": %d, \"nnzL\": %d, \"funits\": %d, \"ftail0\": %d, \"ftail\": %d, \"idx_scale\": %d, \"counts\": [", name.c_str(), k,
           pl.nnzL, pl.funits, pl.ftail0, pl.ftail, sc);
    for (int u = 0; u < pl.funits; ++u) {
      int cnt = 0;
      for (int q = 0; q < 128; ++q) cnt += pl.fmap[(size_t)u * 128 + q] >= 0;
      printf("%s%d", u ? ", " : "", cnt);
    }
    printf("], \"tail\": [");
    for (int i = 0; i < pl.ftail; ++i) {
      printf("%s[", i ? ", " : "");
      bool first = true;
      for (int q = 0; q < 128; ++q) {
        const size_t s = (size_t)(pl.ftail0 + i) * 128 + q;
        if (pl.fmap[s] < 0) continue;
        const unsigned w = (unsigned)pl.fidx[s];
        printf("%s[%d, %d, %d, %d]", first ? "" : ", ", (int)((w & 0xFFFFu) / sc), (int)((w >> 16) / sc), q / 2, q % 2);
        first = false;
      }
      printf("]");
    }
    printf("], \"ftpos\": [");  // per tail unit: slot (lane * 2 + half, -1: none) of rows c0 .. k - 1
    if (pl.ftpos.size() != (size_t)pl.ftail * 64) { fprintf(stderr, "%s: ftpos has %zu entries\n", name.c_str(), pl.ftpos.size()); return 1; }
    for (int i = 0; i < pl.ftail; ++i) {
      printf("%s[", i ? ", " : "");
      for (int ro = 0; ro < 64; ++ro) {
        const int q = pl.ftpos[(size_t)i * 64 + ro];
        printf("%s%d", ro ? ", " : "", q < 0 ? -1 : q - (pl.ftail0 + i) * 128);
      }
      printf("]");
    }
    printf("], \"lcols\": [");
    for (int j = k - 1 - pl.ftail; j < k; ++j) printf("%s%d", j > k - 1 - pl.ftail ? ", " : "", pl.Lp[j + 1] - pl.Lp[j]);
    printf("]}\n");
    prev = std::move(pl);
  }
  fclose(f);
  return 0;
}
