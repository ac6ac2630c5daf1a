// Stand-alone checker of the sparse plan (csrc/sparse_plan.cpp): host code only, its own main.  Built by
// tests/test_sparse_plan_host.py from this file, sparse_plan.cpp and knobs.cpp -- no HIP, no libsfb.so.
//
//   sparse_plan_check ZOOFILE [--only NAME] [--mutate sweep|ustream|supernodal|kmap]
//
// For every pattern of the zoo file (tests/sparse_zoo.py writes it) the plan is built twice, with the default engine and
// with SFB_PLAN_UNITS=0, and per plan
//  (a) the structural invariants of every schedule are checked against the format comments of sparse_plan.h,
//  (b) the schedules are executed the way qp_sparse.hip executes them (sequential doubles, std::fma; build with
//      -ffp-contract=off) and compared bit for bit with a plain reference that knows the original pattern, `perm` and the
//      factor order and nothing else of the plan,
//  (c) one JSON line goes to stdout: the regime fields, and for k <= 400 the solution x of K x = b in the caller's numbering.
// The first violation ends the run with status 1 and a message naming pattern, engine, array and index.
// --mutate corrupts one entry of a built plan (one per schedule family) before the checks: the run must then fail.
#include "../smooth_feedback_amd/csrc/knobs.h"
#include "../smooth_feedback_amd/csrc/sparse_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <set>
#include <string>
#include <vector>

using sfb::SparsePlanHost;
typedef std::vector<int32_t> ivec;
typedef std::vector<double> dvec;

namespace {

constexpr double kSigma = 1e-6, kRho = 0.1;
constexpr int kPad = SparsePlanHost::kSweepPad;

struct Entry {
  std::string name;
  int n = 0, m = 0, ordering = 1, chain = 0;
  bool has_perm = false, has_stage = false;
  ivec Pp, Pi, Ap, Aj, perm, stage;
  dvec Px, Ax, b;  // b: two right-hand sides of k entries, caller's numbering
};

std::string g_where;  // "pattern/engine"

[[noreturn]] void fail(const char *array, long index, const char *fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  fflush(stdout);
  fprintf(stderr, "VIOLATION %s: %s[%ld]: %s\n", g_where.c_str(), array, index, buf);
  exit(1);
}
#define CHECK(cond, array, index, ...) do { if (!(cond)) fail(array, (long)(index), __VA_ARGS__); } while (0)

// ---------------------------------------------------------------------------------------------------------------------
// zoo file: "SFBZOO1\0", int32 count, then per entry
//   int32 len, name, int32 {n, m, ordering, has_perm, has_stage, chain, nnzP, nnzA}, int32 Pp[n+1] Pi[nnzP] Ap[m+1] Aj[nnzA]
//   [perm[k]] [stage[k]], double Px[nnzP] Ax[nnzA] b[2 k]
// chain = 1: the whole-pattern fallback of a pruned plan -- built with the previous entry's perm and lds_doubles
struct Reader {
  FILE *f;
  void raw(void *p, size_t bytes)
  {
    if (bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "zoo file: short read\n"); exit(2); }
  }
  int32_t i32() { int32_t v; raw(&v, 4); return v; }
  ivec ints(size_t c) { if (c > (1u << 26)) { fprintf(stderr, "zoo file: bad count\n"); exit(2); } ivec v(c); raw(v.data(), 4 * c); return v; }
  dvec dbls(size_t c) { if (c > (1u << 26)) { fprintf(stderr, "zoo file: bad count\n"); exit(2); } dvec v(c); raw(v.data(), 8 * c); return v; }
};

std::vector<Entry> read_zoo(const char *path)
{
  FILE *f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  Reader r{f};
  char magic[8];
  r.raw(magic, 8);
  if (memcmp(magic, "SFBZOO1", 8) != 0) { fprintf(stderr, "zoo file: bad magic\n"); exit(2); }
  const int count = r.i32();
  std::vector<Entry> out;
  for (int e = 0; e < count; ++e) {
    Entry z;
    const int len = r.i32();
    if (len < 1 || len > 200) { fprintf(stderr, "zoo file: bad name\n"); exit(2); }
    z.name.resize(len);
    r.raw(&z.name[0], len);
    const ivec h = r.ints(8);
    z.n = h[0]; z.m = h[1]; z.ordering = h[2]; z.has_perm = h[3]; z.has_stage = h[4]; z.chain = h[5];
    if (z.n < 1 || z.m < 1 || h[6] < 0 || h[7] < 0) { fprintf(stderr, "zoo file: bad sizes\n"); exit(2); }
    const size_t k = (size_t)z.n + z.m;
    z.Pp = r.ints(z.n + 1); z.Pi = r.ints(h[6]); z.Ap = r.ints(z.m + 1); z.Aj = r.ints(h[7]);
    if (z.has_perm) z.perm = r.ints(k);
    if (z.has_stage) z.stage = r.ints(k);
    z.Px = r.dbls(h[6]); z.Ax = r.dbls(h[7]); z.b = r.dbls(2 * k);
    out.push_back(std::move(z));
  }
  fclose(f);
  return out;
}

// ---------------------------------------------------------------------------------------------------------------------
// PLAIN REFERENCE.  Knows the original pattern and values, `perm` and the factor order (F column j = unknown
// perm[f2s[j]]); shares nothing else with the plan.
struct Ref {
  int k = 0;
  std::vector<std::vector<std::pair<int, double>>> col;  // strictly lower part of L in F, rows ascending
  dvec D;
  dvec x[2];  // caller's numbering
};

// KKT matrix [P + sigma I, A'; A, -1/rho I] of the upper-stored part of P (qp_solver.hpp:382-395), unscaled
void kkt_entries(const Entry &z, std::vector<std::map<int, double>> &lowerF, const ivec &rankOfOrig)
{
  const int n = z.n, m = z.m, k = n + m;
  lowerF.assign(k, {});
  auto put = [&](int r, int c, double v) {
    const int a = rankOfOrig[r], b = rankOfOrig[c];
    lowerF[std::min(a, b)][std::max(a, b)] = v;
  };
  std::vector<char> hasdiag(n, 0);
  for (int c = 0; c < n; ++c)
    for (int p = z.Pp[c]; p < z.Pp[c + 1]; ++p)
      if (z.Pi[p] < c) put(z.Pi[p], c, z.Px[p]);
      else if (z.Pi[p] == c) { put(c, c, z.Px[p] + kSigma); hasdiag[c] = 1; }
  for (int c = 0; c < n; ++c)
    if (!hasdiag[c]) put(c, c, kSigma);
  for (int r = 0; r < m; ++r) {
    for (int p = z.Ap[r]; p < z.Ap[r + 1]; ++p) put(z.Aj[p], n + r, z.Ax[p]);
    put(n + r, n + r, -1.0 / kRho);
  }
}

void reference(const Entry &z, const ivec &perm, const ivec &f2s, Ref &R)
{
  const int k = z.n + z.m;
  R.k = k;
  ivec rankOfOrig(k);
  for (int j = 0; j < k; ++j) rankOfOrig[perm[f2s[j]]] = j;
  std::vector<std::map<int, double>> K;
  kkt_entries(z, K, rankOfOrig);
  // left-looking column LDL': column j receives its sources s < j in ascending order, each one
  //   work(i) = fma(-L(i, s), L(j, s) D(s), work(i)),  i >= j;  the pattern grows by the fill as it goes
  R.col.assign(k, {});
  R.D.assign(k, 0.0);
  std::vector<std::vector<std::pair<int, int>>> srcs(k);  // row j -> (s, position of (j, s) in col[s]), s ascending
  dvec work(k, 0.0);
  ivec mark(k, -1), pat;
  for (int j = 0; j < k; ++j) {
    pat.clear();
    for (const auto &e : K[j]) {
      work[e.first] = e.second;
      if (e.first > j && mark[e.first] != j) { mark[e.first] = j; pat.push_back(e.first); }
    }
    for (const auto &sp : srcs[j]) {
      const auto &cs = R.col[sp.first];
      const double mult = cs[sp.second].second * R.D[sp.first];
      for (size_t e = sp.second; e < cs.size(); ++e) {
        const int i = cs[e].first;
        if (i > j && mark[i] != j) { mark[i] = j; pat.push_back(i); }
        work[i] = std::fma(-cs[e].second, mult, work[i]);
      }
    }
    R.D[j] = work[j];
    work[j] = 0.0;
    CHECK(R.D[j] != 0.0, "reference D", j, "zero pivot in the plain reference");
    std::sort(pat.begin(), pat.end());
    for (int i : pat) {
      srcs[i].emplace_back(j, (int)R.col[j].size());
      R.col[j].emplace_back(i, work[i] / R.D[j]);
      work[i] = 0.0;
    }
  }
  // the same once more on a dense matrix with no notion of a pattern at all (every s < j is a source; absent entries
  // contribute exact zeros), for the sizes where that is affordable
  if (k <= 1100) {
    dvec M((size_t)k * k, 0.0);  // column-major lower
    for (int j = 0; j < k; ++j)
      for (const auto &e : K[j]) M[(size_t)j * k + e.first] = e.second;
    dvec Dd(k);
    for (int j = 0; j < k; ++j) {
      double *cj = &M[(size_t)j * k];
      for (int s = 0; s < j; ++s) {
        const double *cs = &M[(size_t)s * k];
        if (cs[j] == 0.0) continue;  // (an exact zero multiplier changes no value, only signs of zeros)
        const double mult = cs[j] * Dd[s];
        for (int i = j; i < k; ++i) cj[i] = std::fma(-cs[i], mult, cj[i]);
      }
      Dd[j] = cj[j];
      for (int i = j + 1; i < k; ++i) cj[i] = cj[i] / Dd[j];
    }
    for (int j = 0; j < k; ++j) {
      CHECK(Dd[j] == R.D[j], "reference D", j, "dense and column-list references differ: %.17g vs %.17g", Dd[j], R.D[j]);
      size_t e = 0;
      for (int i = j + 1; i < k; ++i) {
        double v = 0.0;
        if (e < R.col[j].size() && R.col[j][e].first == i) v = R.col[j][e++].second;
        CHECK(M[(size_t)j * k + i] == v, "reference L", (long)j * k + i, "dense and column-list references differ");
      }
    }
  }
  // textbook triangular solves in the sweeps' numbering S (S index of F column j = f2s[j]):
  //   forward by columns ascending, t = t / D as a multiplication by 1 / D (qp_solver.hpp:458), backward by rows descending
  std::vector<std::vector<std::pair<int, double>>> colS(k), rowS(k);
  for (int j = 0; j < k; ++j)
    for (const auto &e : R.col[j]) {
      const int cS = f2s[j], rS = f2s[e.first];
      CHECK(rS > cS, "factor order", j, "an entry of L is above the diagonal in the sweeps' numbering");
      colS[cS].emplace_back(rS, e.second);
      rowS[rS].emplace_back(cS, e.second);
    }
  for (auto &c : colS) std::sort(c.begin(), c.end());
  for (int rhs = 0; rhs < 2; ++rhs) {
    dvec t(k);
    for (int i = 0; i < k; ++i) t[i] = z.b[(size_t)rhs * k + perm[i]];
    for (int j = 0; j < k; ++j)
      for (const auto &e : colS[j]) t[e.first] = std::fma(-e.second, t[j], t[e.first]);
    for (int j = 0; j < k; ++j) t[f2s[j]] = (1.0 / R.D[j]) * t[f2s[j]];
    for (int j = k - 1; j >= 0; --j)
      for (const auto &e : rowS[j]) t[e.first] = std::fma(-e.second, t[j], t[e.first]);
    R.x[rhs].assign(k, 0.0);
    for (int i = 0; i < k; ++i) R.x[rhs][perm[i]] = t[i];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// What the checker derives from the plan's pattern of L (Lp, Li in S) and f2s: the pattern in F and, per F position,
// the entry it holds.
struct Derived {
  int k = 0, nnzL = 0;
  ivec rankF, FLp, FLi, Fcol, posF;  // posF[S position] = F position
  ivec SrowOfF, ScolOfF;
  int pos(int col, int row) const
  {
    const int32_t *b = FLi.data() + FLp[col], *e = FLi.data() + FLp[col + 1];
    const int32_t *it = std::lower_bound(b, e, row);
    return (it != e && *it == row) ? (int)(it - FLi.data()) : -1;
  }
  int acc(int a, int b) const { return a == b ? nnzL + b : pos(b, a); }  // accumulator of the pair a >= b
};

void derive(const SparsePlanHost &pl, Derived &d)
{
  const int k = pl.k;
  d.k = k;
  d.nnzL = pl.nnzL;
  CHECK((int)pl.perm.size() == k && (int)pl.pinv.size() == k && (int)pl.f2s.size() == k, "perm", 0, "size");
  std::vector<char> seen(k, 0);
  for (int i = 0; i < k; ++i) {
    CHECK(pl.perm[i] >= 0 && pl.perm[i] < k && !seen[pl.perm[i]], "perm", i, "not a permutation");
    seen[pl.perm[i]] = 1;
    CHECK(pl.pinv[pl.perm[i]] == i, "pinv", pl.perm[i], "not the inverse of perm");
  }
  d.rankF.assign(k, -1);
  for (int j = 0; j < k; ++j) {
    CHECK(pl.f2s[j] >= 0 && pl.f2s[j] < k && d.rankF[pl.f2s[j]] < 0, "f2s", j, "not a permutation");
    d.rankF[pl.f2s[j]] = j;
  }
  CHECK((int)pl.Lp.size() == k + 1 && pl.Lp[0] == 0 && pl.Lp[k] == pl.nnzL && (int)pl.Li.size() == pl.nnzL, "Lp", k, "size");
  d.FLp.assign(k + 1, 0);
  d.FLi.resize(pl.nnzL); d.Fcol.resize(pl.nnzL); d.posF.resize(pl.nnzL); d.SrowOfF.resize(pl.nnzL); d.ScolOfF.resize(pl.nnzL);
  std::vector<std::pair<int32_t, int32_t>> tmp;
  for (int jF = 0; jF < k; ++jF) {
    const int jS = pl.f2s[jF];
    CHECK(pl.Lp[jS + 1] >= pl.Lp[jS], "Lp", jS, "not monotone");
    tmp.clear();
    for (int p = pl.Lp[jS]; p < pl.Lp[jS + 1]; ++p) {
      CHECK(pl.Li[p] > jS && pl.Li[p] < k && (p == pl.Lp[jS] || pl.Li[p] > pl.Li[p - 1]), "Li", p, "rows of a column must ascend below the diagonal");
      tmp.emplace_back(d.rankF[pl.Li[p]], p);
    }
    std::sort(tmp.begin(), tmp.end());
    d.FLp[jF + 1] = d.FLp[jF] + (int)tmp.size();
    for (size_t e = 0; e < tmp.size(); ++e) {
      const int x = d.FLp[jF] + (int)e;
      CHECK(tmp[e].first > jF, "f2s", jF, "the factor order puts a row of column %d above it", jF);
      d.FLi[x] = tmp[e].first; d.Fcol[x] = jF; d.posF[tmp[e].second] = x;
      d.SrowOfF[x] = pl.Li[tmp[e].second]; d.ScolOfF[x] = jS;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// (a) structural invariants
void check_sweep(const SparsePlanHost &pl, const Derived &d, const bool forward)
{
  const int k = pl.k, sc = pl.idx_scale;
  const ivec &xmap = forward ? pl.fmap : pl.bmap, &xidx = forward ? pl.fidx : pl.bidx, &xmask = forward ? pl.fmask : pl.bmask;
  const int units = forward ? pl.funits : pl.bunits, full0 = forward ? pl.ffull0 : pl.bfull0, full1 = forward ? pl.ffull1 : pl.bfull1;
  const char *nm = forward ? "fmap" : "bmap", *ni = forward ? "fidx" : "bidx", *nk = forward ? "fmask" : "bmask";
  // (the kernel runs the sweeps and builds their copies in whole prefetch blocks of 8 units: sparse_plan.cpp, qp_sparse.hip sweep_dev)
  CHECK(units >= 0 && units % 8 == 0, forward ? "funits" : "bunits", units, "unit count must be a multiple of 8");
  const size_t total = (size_t)(units + kPad) * 128;
  CHECK(xmap.size() == total && xidx.size() == total, nm, xmap.size(), "size: %zu slots expected (units + kSweepPad padding units)", total);
  CHECK(xmask.size() == (size_t)units + 2 * kPad, nk, xmask.size(), "size");
  CHECK(full0 % 8 == 0 && full1 % 8 == 0 && 0 <= full0 && full0 <= full1 && full1 <= units, forward ? "ffull" : "bfull", full0, "[full0, full1) = [%d, %d)", full0, full1);
  std::vector<char> seen(pl.nnzL, 0);
  ivec remaining(k + 1, 0), last(k + 1, forward ? -1 : k), stampT(k + 1, -1), stampP(k + 1, -1);
  for (int x = 0; x < pl.nnzL; ++x) remaining[forward ? d.SrowOfF[x] : d.ScolOfF[x]]++;
  long nreal = 0;
  for (int u = 0; u < units + kPad; ++u) {
    int cnt = 0, top_lane = -1;
    for (int l = 0; l < 64; ++l)
      for (int s = 0; s < 2; ++s) {
        const size_t q = ((size_t)u * 64 + l) * 2 + s;
        const unsigned w = (unsigned)xidx[q], lo = w & 0xFFFFu, hi = w >> 16;
        CHECK(lo % sc == 0 && hi % sc == 0, ni, q, "offset is no multiple of idx_scale %d", sc);
        const int tgt = (int)(lo / sc), piv = (int)(hi / sc);
        CHECK(tgt <= k && piv <= k, ni, q, "target %d / pivot %d outside the work vector of k + 1 = %d", tgt, piv, k + 1);
        if (xmap[q] < 0) {
          CHECK(xmap[q] == -1 && tgt == k && piv == k, ni, q, "padding slot must have map -1 and target = pivot = k");
          continue;
        }
        CHECK(u < units, nm, q, "real slot in a padding unit");
        const int x = xmap[q];
        CHECK(x < pl.nnzL, nm, q, "position %d outside L", x);
        CHECK(!seen[x], nm, q, "position %d of L occurs twice", x);
        seen[x] = 1;
        const int wt = forward ? d.SrowOfF[x] : d.ScolOfF[x], wp = forward ? d.ScolOfF[x] : d.SrowOfF[x];
        CHECK(tgt == wt && piv == wp, ni, q, "slot of L position %d has (target, pivot) (%d, %d), the entry is (%d, %d)", x, tgt, piv, wt, wp);
        CHECK(stampT[piv] != u, ni, q, "pivot %d is a target of the same unit", piv);
        CHECK(remaining[piv] == 0, ni, q, "pivot %d has not received all its updates in earlier units", piv);
        CHECK(stampT[tgt] != u, ni, q, "two slots of unit %d share target %d", u, tgt);
        CHECK(stampP[tgt] != u, ni, q, "target %d is a pivot of the same unit", tgt);
        CHECK(forward ? piv > last[tgt] : piv < last[tgt], ni, q, "updates of target %d leave the sequential order", tgt);
        last[tgt] = piv;
        stampT[tgt] = u; stampP[piv] = u;
        ++cnt; ++nreal;
        top_lane = std::max(top_lane, l);
      }
    for (int l = 0; l < 64; ++l)  // (after the unit: its targets have one update less to come)
      for (int s = 0; s < 2; ++s) {
        const size_t q = ((size_t)u * 64 + l) * 2 + s;
        if (xmap[q] >= 0) remaining[((unsigned)xidx[q] & 0xFFFFu) / sc]--;
      }
    const int lanes = std::max(1, (cnt + 1) / 2);
    CHECK(xmask[u] == 64 - lanes, nk, u, "mask %d, the unit has %d slots (64 - leading lanes = %d)", xmask[u], cnt, 64 - lanes);
    CHECK(top_lane < lanes, nk, u, "a slot sits in lane %d, behind the %d leading lanes the value load fetches", top_lane, lanes);
    if (u >= full0 && u < full1) CHECK(cnt == 128, forward ? "ffull" : "bfull", u, "unit inside the full run has %d slots", cnt);
  }
  for (size_t u = units; u < xmask.size(); ++u) CHECK(xmask[u] == 63, nk, u, "padding unit must load lane 0 only");
  for (int x = 0; x < pl.nnzL; ++x) CHECK(seen[x], nm, x, "position %d of L occurs in no slot", x);
  CHECK(nreal == pl.nnzL, nm, nreal, "slot count");
}

struct SegV { int a0, a1, c0, c1, lds, nL, accN, kp0, kp1, gL, nout, omap0; };

std::vector<SegV> check_segments(const SparsePlanHost &pl, const Derived &d, const ivec &FKp)
{
  const int k = pl.k;
  CHECK(pl.nseg >= 1 && (int)pl.seg.size() == pl.nseg * SparsePlanHost::kSegStride, "seg", pl.seg.size(), "size");
  std::vector<SegV> segs;
  int c = 0, a = 0;
  for (int s = 0; s < pl.nseg; ++s) {
    const int32_t *p = &pl.seg[(size_t)s * 12];
    SegV g{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11]};
    CHECK(g.c0 == c && g.c1 > g.c0 && g.c1 <= k, "seg", 12 * s + 2, "segments must partition [0, k) in ascending order");
    CHECK(g.a0 == a && g.a1 >= g.a0, "seg", 12 * s, "unit / supernode ranges must follow each other");
    CHECK(g.lds == 0 || g.lds == 1, "seg", 12 * s + 4, "lds flag");
    CHECK(g.kp0 == FKp[g.c0] && g.kp1 == FKp[g.c1], "seg", 12 * s + 7, "K entry range");
    if (pl.units || g.lds) {
      CHECK(g.gL == d.FLp[g.c0] && g.nL == d.FLp[g.c1] - d.FLp[g.c0] && g.accN == g.nL + g.c1 - g.c0, "seg", 12 * s + 5, "nL / accN / first L entry");
    }
    if (pl.units) {
      CHECK(g.nout >= 0 && g.omap0 >= 0 && (size_t)g.omap0 + g.nout + 512 <= pl.uomap.size(), "seg", 12 * s + 10, "outside map range");
      CHECK(g.accN + g.nout + 3 <= pl.lds_doubles, "seg", 12 * s + 6, "accN + nout + 3 = %d > lds_doubles %d", g.accN + g.nout + 3, pl.lds_doubles);
    } else if (g.lds) {
      CHECK(((g.accN + 3) & ~1) <= pl.lds_doubles, "seg", 12 * s + 6, "accumulators do not fit the LDS");
    }
    c = g.c1; a = g.a1;
    segs.push_back(g);
  }
  CHECK(c == k, "seg", 12 * (pl.nseg - 1) + 3, "segments end at column %d of %d", c, k);
  CHECK(a == (pl.units ? pl.nunits : pl.nsn), "seg", 12 * (pl.nseg - 1) + 1, "unit / supernode ranges end at %d", a);
  // ztop: exactly the accumulators of the open segments, then {sink, zero}
  ivec want;
  for (const SegV &g : segs)
    if (!g.lds) { want.insert(want.end(), {d.FLp[g.c0], d.FLp[g.c1] - d.FLp[g.c0], pl.nnzL + g.c0, g.c1 - g.c0}); }
  want.insert(want.end(), {pl.nnzL + k, 2});
  CHECK(pl.ztop == want && pl.nztop == (int)want.size() / 2, "ztop", 0, "must cover exactly the accumulators of the open segments and {sink, zero}");
  return segs;
}

// segment of an accumulator (by the column that owns it)
int seg_of_acc(const std::vector<SegV> &segs, const Derived &d, int g)
{
  const int col = g < d.nnzL ? d.Fcol[g] : g - d.nnzL;
  for (size_t s = 0; s < segs.size(); ++s)
    if (col >= segs[s].c0 && col < segs[s].c1) return (int)s;
  return -1;
}

void check_kmaps(const Entry &z, const SparsePlanHost &pl, const Derived &d, const std::vector<SegV> &segs, const ivec &FKp)
{
  const int n = z.n, k = pl.k, nnzK = pl.nnzK;
  CHECK(pl.Kmap.size() == (size_t)nnzK + 512 && pl.KmapL.size() == (size_t)nnzK + 512 && pl.Kdesc.size() == 4 * ((size_t)nnzK + 512), "Kmap", pl.Kmap.size(), "size (padded by 512)");
  // every entry of the KKT matrix exactly once
  std::set<std::pair<int, int>> want, got;
  std::vector<char> hasdiag(n, 0);
  for (int c = 0; c < n; ++c)
    for (int p = z.Pp[c]; p < z.Pp[c + 1]; ++p)
      if (z.Pi[p] <= c) { want.insert({sfb::K_P, p}); if (z.Pi[p] == c) hasdiag[c] = 1; }
  for (int c = 0; c < n; ++c)
    if (!hasdiag[c]) want.insert({sfb::K_SIGMA, c});
  for (int p = 0; p < z.Ap[z.m]; ++p) want.insert({sfb::K_A, p});
  for (int r = 0; r < z.m; ++r) want.insert({sfb::K_RHO, r});
  CHECK((int)want.size() == nnzK, "Kdesc", nnzK, "nnzK %d, the KKT matrix has %zu entries", nnzK, want.size());
  std::vector<char> used(pl.nnzL + k, 0);
  size_t nt = 0;
  for (size_t s = 0; s < segs.size(); ++s)
    for (int p = segs[s].kp0; p < segs[s].kp1; ++p) {
      const int kind = pl.Kdesc[4 * (size_t)p], idx = pl.Kdesc[4 * (size_t)p + 1], r = pl.Kdesc[4 * (size_t)p + 2], c = pl.Kdesc[4 * (size_t)p + 3];
      CHECK(kind >= 0 && kind <= 3 && want.count({kind, idx}), "Kdesc", 4 * (size_t)p, "no entry of the KKT matrix: kind %d index %d", kind, idx);
      CHECK(got.insert({kind, idx}).second, "Kdesc", 4 * (size_t)p, "KKT entry (kind %d, index %d) occurs twice", kind, idx);
      int orow, ocol;  // the entry in the caller's KKT numbering
      if (kind == sfb::K_P) {
        CHECK(r == z.Pi[idx] && z.Pp[c] <= idx && idx < z.Pp[c + 1], "Kdesc", 4 * (size_t)p + 2, "row / column of the P entry");
        orow = r; ocol = c;
      } else if (kind == sfb::K_A) {
        CHECK(c == z.Aj[idx] && z.Ap[r] <= idx && idx < z.Ap[r + 1], "Kdesc", 4 * (size_t)p + 2, "row / column of the A entry");
        orow = n + r; ocol = c;
      } else if (kind == sfb::K_SIGMA) orow = ocol = idx;
      else orow = ocol = n + idx;
      const int a = d.rankF[pl.pinv[orow]], b = d.rankF[pl.pinv[ocol]];
      const int g = d.acc(std::max(a, b), std::min(a, b));
      CHECK(g >= 0 && pl.Kmap[p] == g, "Kmap", p, "accumulator %d, the entry (%d, %d) of the factor numbering lives in %d", pl.Kmap[p], std::max(a, b), std::min(a, b), g);
      CHECK(std::min(a, b) >= segs[s].c0 && std::min(a, b) < segs[s].c1, "Kmap", p, "entry of column %d listed with segment %zu", std::min(a, b), s);
      CHECK(!used[g], "Kmap", p, "two KKT entries share accumulator %d", g);
      used[g] = 1;
      if (segs[s].lds) {
        const int off = g < pl.nnzL ? g - segs[s].gL : segs[s].nL + (g - pl.nnzL - segs[s].c0);
        CHECK(pl.KmapL[p] == off && off >= 0 && off < segs[s].accN, "KmapL", p, "LDS offset %d, accumulator %d sits at %d of the segment's %d", pl.KmapL[p], g, off, segs[s].accN);
      } else {
        CHECK(nt < pl.KmapT.size() && pl.KmapT[nt] == g, "KmapT", nt, "accumulator of the top entry");
        for (int e = 0; e < 4; ++e) CHECK(pl.KdescT[4 * nt + e] == pl.Kdesc[4 * (size_t)p + e], "KdescT", 4 * nt + e, "descriptor of the top entry");
        ++nt;
      }
    }
  CHECK((int)got.size() == nnzK && FKp[k] == nnzK, "Kdesc", nnzK, "entries listed: %zu of %d", got.size(), nnzK);
  CHECK((int)nt == pl.nnzKT && pl.KmapT.size() == nt + 512 && pl.KdescT.size() == 4 * (nt + 512), "KmapT", nt, "nnzKT / padding");
  for (size_t p = nt; p < nt + 512; ++p) CHECK(pl.KmapT[p] == pl.nnzL + k && pl.KdescT[4 * p] == sfb::K_SIGMA, "KmapT", p, "padding goes to the sink as a constant");
  for (size_t p = nnzK; p < (size_t)nnzK + 512; ++p) CHECK(pl.Kmap[p] == pl.nnzL + k && pl.Kdesc[4 * p] == sfb::K_SIGMA, "Kmap", p, "padding goes to the sink as a constant");
}

void check_units(const SparsePlanHost &pl, const Derived &d, const std::vector<SegV> &segs)
{
  const int nnzL = pl.nnzL, k = pl.k;
  CHECK((size_t)pl.lds_doubles * 8 < 65536, "lds_doubles", pl.lds_doubles, "byte offsets of the unit engine need 16 bits");
  CHECK(pl.ustream.size() == ((size_t)pl.nunits + 2 * kPad) * 256, "ustream", pl.ustream.size(), "size (padded by two blocks)");
  CHECK(pl.utype.size() == (size_t)pl.nunits + kPad + 32, "utype", pl.utype.size(), "size");
  for (size_t q = (size_t)pl.nunits * 256; q < pl.ustream.size(); ++q) CHECK(pl.ustream[q] == 0, "ustream", q, "trailing padding");
  for (size_t u = pl.nunits; u < pl.utype.size(); ++u) CHECK(pl.utype[u] == 0, "utype", u, "trailing padding");
  size_t omap_end = 0;
  std::vector<char> closedAcc(nnzL + k, 0);
  for (const SegV &g : segs)
    if (g.lds) {
      std::fill(closedAcc.begin() + g.gL, closedAcc.begin() + g.gL + g.nL, 1);
      std::fill(closedAcc.begin() + nnzL + g.c0, closedAcc.begin() + nnzL + g.c1, 1);
    }
  ivec stampW(pl.lds_doubles, -1), stampR(pl.lds_doubles, -1);
  for (size_t si = 0; si < segs.size(); ++si) {
    const SegV &g = segs[si];
    CHECK((size_t)g.omap0 == omap_end, "seg", 12 * si + 11, "outside maps must follow each other");
    omap_end += g.nout;
    const int SINK = g.accN + g.nout, ZERO = SINK + 1, ONE = SINK + 2;
    std::set<int> distinct;
    for (int e = 0; e < g.nout; ++e) {
      const int a = pl.uomap[g.omap0 + e];
      CHECK(a >= 0 && a < nnzL + k, "uomap", g.omap0 + e, "accumulator %d out of range", a);
      CHECK(distinct.insert(a).second, "uomap", g.omap0 + e, "accumulator %d fetched twice by one segment", a);
      const int col = a < nnzL ? d.Fcol[a] : a - nnzL;
      CHECK(col >= g.c1, "uomap", g.omap0 + e, "outside accumulator %d belongs to column %d, not behind the segment [%d, %d)", a, col, g.c0, g.c1);
      CHECK(!closedAcc[a], "uomap", g.omap0 + e, "accumulator %d belongs to a closed segment (a whole subtree: nobody outside updates it)", a);
    }
    // every division and every update of the segment's columns exactly once
    std::vector<char> dm_seen(g.nL, 0), out_used(g.nout, 0);
    std::set<std::pair<int, int>> f_seen;  // (L position of a, L position of b)
    long nF = 0;
    for (int u = g.a0; u < g.a1; ++u) {
      const int32_t *us = &pl.ustream[(size_t)u * 256];
      const bool dm = us[1] == -1;
      CHECK(pl.utype[u] == (dm ? 1 : 0), "utype", u, "disagrees with the stream's second word");
      for (int l = 0; l < 64; ++l)
        for (int h = 0; h < 2; ++h) {
          const size_t q = (size_t)u * 256 + (size_t)l * 4 + 2 * h;
          const unsigned w0 = (unsigned)pl.ustream[q], w1 = (unsigned)pl.ustream[q + 1];
          CHECK((w1 == 0xFFFFFFFFu) == dm, "ustream", q + 1, "a unit holds slots of one kind");
          unsigned off[4] = {w0 & 0xFFFFu, w0 >> 16, dm ? 0u : (w1 & 0xFFFFu), dm ? 0u : (w1 >> 16)};
          for (int e = 0; e < (dm ? 2 : 4); ++e)
            CHECK(off[e] % 8 == 0 && off[e] < 8u * (unsigned)pl.lds_doubles, "ustream", q + e / 2, "byte offset %u outside the LDS of %d doubles", off[e], pl.lds_doubles);
          const int T = off[0] / 8;
          if (T == SINK) {  // padding
            if (dm) CHECK((int)off[1] / 8 == ONE, "ustream", q, "padding division must be {SINK, ONE}");
            else CHECK((int)off[1] / 8 == ZERO && (int)off[2] / 8 == ZERO && (int)off[3] / 8 == ZERO, "ustream", q, "padding update must be {SINK, ZERO, ZERO, ZERO}");
            continue;
          }
          CHECK(T < SINK, "ustream", q, "target offset %d behind the sink %d", T, SINK);
          CHECK(stampW[T] != u, "ustream", q, "two slots of unit %d write offset %d", u, T);
          CHECK(stampR[T] != u, "ustream", q, "offset %d is written and read in unit %d", T, u);
          stampW[T] = u;
          const int nops = dm ? 1 : 3;
          for (int e = 1; e <= nops; ++e) {
            const int o = off[dm ? 1 : e] / 8;
            CHECK(o < SINK, "ustream", q, "real slot reads the padding operand %d", o);
            CHECK(stampW[o] != u, "ustream", q, "offset %d is written and read in unit %d", o, u);
            stampR[o] = u;
          }
          if (dm) {
            const int D = off[1] / 8;
            CHECK(T < g.nL && D >= g.nL && D < g.accN, "ustream", q, "division L(%d) / D(%d): operands outside their ranges", T, D);
            CHECK(d.Fcol[g.gL + T] == g.c0 + (D - g.nL), "ustream", q, "division of an entry of column %d by D of column %d", d.Fcol[g.gL + T], g.c0 + (D - g.nL));
            CHECK(!dm_seen[T], "ustream", q, "entry %d divided twice", T);
            dm_seen[T] = 1;
          } else {
            const int A = off[1] / 8, B = off[2] / 8, D = off[3] / 8;
            CHECK(A < g.nL && B < g.nL && D >= g.nL && D < g.accN, "ustream", q, "update operands outside their ranges");
            const int j = g.c0 + (D - g.nL), pa = g.gL + A, pb = g.gL + B;
            CHECK(d.Fcol[pa] == j && d.Fcol[pb] == j, "ustream", q, "operands of columns %d, %d with D of column %d", d.Fcol[pa], d.Fcol[pb], j);
            const int ra = d.FLi[pa], rb = d.FLi[pb];
            CHECK(ra >= rb, "ustream", q, "pair (a, b) = (%d, %d): a >= b expected", ra, rb);
            const int acc = d.acc(ra, rb);
            CHECK(acc >= 0, "ustream", q, "pair (%d, %d) has no accumulator", ra, rb);
            int want;
            if (rb < g.c1) want = acc < nnzL ? acc - g.gL : g.nL + (rb - g.c0);
            else {
              CHECK(T >= g.accN, "ustream", q, "update of a later column must go to an outside accumulator");
              CHECK(pl.uomap[g.omap0 + T - g.accN] == acc, "uomap", g.omap0 + T - g.accN, "outside accumulator %d, the pair (%d, %d) updated through it lives in %d", pl.uomap[g.omap0 + T - g.accN], ra, rb, acc);
              out_used[T - g.accN] = 1;
              want = T;
            }
            CHECK(T == want, "ustream", q, "update of pair (%d, %d) targets offset %d, its accumulator sits at %d", ra, rb, T, want);
            CHECK(f_seen.insert({pa, pb}).second, "ustream", q, "update (%d, %d) of column %d occurs twice", ra, rb, j);
            ++nF;
          }
        }
    }
    long wantF = 0;
    for (int j = g.c0; j < g.c1; ++j) { const long c = d.FLp[j + 1] - d.FLp[j]; wantF += c * (c + 1) / 2; }
    CHECK(nF == wantF, "ustream", (size_t)g.a0 * 256, "segment %zu has %ld updates, its columns need %ld", si, nF, wantF);
    for (int e = 0; e < g.nL; ++e) CHECK(dm_seen[e], "ustream", (size_t)g.a0 * 256, "entry %d of segment %zu is never divided", e, si);
    for (int e = 0; e < g.nout; ++e) CHECK(out_used[e], "uomap", g.omap0 + e, "fetched and never updated");
  }
  CHECK(pl.uomap.size() == omap_end + 512, "uomap", pl.uomap.size(), "size (padded by 512)");
  for (size_t e = omap_end; e < pl.uomap.size(); ++e) CHECK(pl.uomap[e] == nnzL + k, "uomap", e, "padding must be the sink");
}

void check_supernodes(const SparsePlanHost &pl, const Derived &d, const std::vector<SegV> &segs)
{
  const int nnzL = pl.nnzL, k = pl.k, SCRATCH = nnzL + k, ZERO = nnzL + k + 1;
  CHECK(pl.ustream.empty() && pl.utype.empty() && pl.uomap.empty() && pl.nunits == 0, "ustream", 0, "unit arrays of a supernodal plan must be empty");
  CHECK((int)pl.snptr.size() == pl.nsn + 1 && (int)pl.snR.size() == pl.nsn && (int)pl.poff.size() == pl.nsn + 1 && (int)pl.rptr.size() == pl.nsn + 1 &&
        (int)pl.rsplit.size() == pl.nsn + 1, "snptr", pl.nsn, "sizes");
  CHECK(pl.snptr[pl.nsn] == k && pl.rptr[0] == 0 && pl.rptr[pl.nsn] == pl.rsteps, "snptr", pl.nsn, "ends");
  const size_t npm = pl.poff[pl.nsn], nrt = (size_t)pl.rsteps * 64;
  CHECK(pl.pmap.size() == npm + 64 * kPad && pl.pmapL.size() == pl.pmap.size(), "pmap", pl.pmap.size(), "size (padded)");
  CHECK(pl.rtgt.size() == nrt + 64 * kPad && pl.rab.size() == pl.rtgt.size(), "rtgt", pl.rtgt.size(), "size (padded)");
  for (size_t q = npm; q < pl.pmap.size(); ++q) CHECK(pl.pmap[q] == SCRATCH && pl.pmapL[q] == 0, "pmap", q, "padding");
  for (size_t q = nrt; q < pl.rtgt.size(); ++q) CHECK(pl.rtgt[q] == SCRATCH && pl.rab[q] == 0, "rtgt", q, "padding");
  std::vector<char> closedAcc(nnzL + k, 0);
  for (const SegV &g : segs)
    if (g.lds) {
      std::fill(closedAcc.begin() + g.gL, closedAcc.begin() + g.gL + g.nL, 1);
      std::fill(closedAcc.begin() + nnzL + g.c0, closedAcc.begin() + nnzL + g.c1, 1);
    }
  int maxcol = 0;
  for (int j = 0; j < k; ++j) maxcol = std::max(maxcol, d.FLp[j + 1] - d.FLp[j]);
  CHECK(pl.maxcol == maxcol, "maxcol", 0, "%d, the longest column has %d", pl.maxcol, maxcol);
  for (size_t si = 0; si < segs.size(); ++si) {
    const SegV &g = segs[si];
    CHECK(g.a1 > g.a0 && pl.snptr[g.a0] == g.c0 && pl.snptr[g.a1] == g.c1, "snptr", g.a0, "supernodes of segment %zu must cover its columns", si);
    const int scratch = g.lds ? pl.lds_doubles - ((g.accN + 3) & ~1) : pl.lds_doubles;
    auto lds_off = [&](int a) {
      if (a == SCRATCH) return g.accN;
      if (a == ZERO) return g.accN + 1;
      if (a < nnzL) return (a >= g.gL && a < g.gL + g.nL) ? a - g.gL : -1;
      return (a - nnzL >= g.c0 && a - nnzL < g.c1) ? g.nL + (a - nnzL - g.c0) : -1;
    };
    for (int sn = g.a0; sn < g.a1; ++sn) {
      const int j0 = pl.snptr[sn], w = pl.snptr[sn + 1] - j0, R = pl.snR[sn];
      CHECK(w >= 1 && w <= 16 && j0 + w <= g.c1, "snptr", sn, "members must be 1..16 consecutive columns of one segment");
      ivec U;  // union of the members' structures behind the panel's own columns
      for (int jj = 0; jj < w; ++jj)
        for (int p = d.FLp[j0 + jj]; p < d.FLp[j0 + jj + 1]; ++p)
          if (d.FLi[p] >= j0 + w) U.push_back(d.FLi[p]);
      std::sort(U.begin(), U.end());
      U.erase(std::unique(U.begin(), U.end()), U.end());
      const int nu = (int)U.size();
      CHECK(R == w + nu, "snR", sn, "panel rows %d, members %d + union %d", R, w, nu);
      CHECK(2 * w * R <= scratch, "snR", sn, "panel and multipliers 2 w R = %d do not fit the scratch of %d doubles", 2 * w * R, scratch);
      if (g.lds) CHECK(R <= 64, "snR", sn, "on-chip panels are eliminated in registers: R = %d > 64", R);
      CHECK(pl.poff[sn + 1] - pl.poff[sn] == w * R, "poff", sn, "panel map length");
      for (int jj = 0; jj < w; ++jj)
        for (int r = 0; r < R; ++r) {
          const size_t q = (size_t)pl.poff[sn] + (size_t)jj * R + r;
          int want = SCRATCH;
          if (r == jj) want = nnzL + j0 + jj;
          else if (r > jj) { const int pos = d.pos(j0 + jj, r < w ? j0 + r : U[r - w]); want = pos >= 0 ? pos : ZERO; }
          CHECK(pl.pmap[q] == want, "pmap", q, "accumulator %d, panel entry (row %d, member %d) lives in %d", pl.pmap[q], r, jj, want);
          CHECK(pl.pmapL[q] == (g.lds ? lds_off(want) : 0) && pl.pmapL[q] >= 0, "pmapL", q, "LDS offset of the panel entry");
        }
      // trailing schedule: every pair (a >= b) of U that some member updates, exactly once
      CHECK(pl.rptr[sn] <= pl.rsplit[sn] && pl.rsplit[sn] <= pl.rptr[sn + 1], "rsplit", sn, "outside [rptr, rptr + 1]");
      if (!g.lds) CHECK(pl.rsplit[sn] == pl.rptr[sn], "rsplit", sn, "a top segment has no on-chip steps");
      std::map<int, std::pair<int, int>> want;  // accumulator -> (a, b) positions in U
      for (int bq = 0; bq < nu; ++bq)
        for (int aq = bq; aq < nu; ++aq) {
          bool touched = false;
          for (int jj = 0; jj < w && !touched; ++jj) touched = d.pos(j0 + jj, U[aq]) >= 0 && d.pos(j0 + jj, U[bq]) >= 0;
          if (!touched) continue;
          const int acc = d.acc(U[aq], U[bq]);
          CHECK(acc >= 0, "rtgt", (size_t)pl.rptr[sn] * 64, "members of supernode %d update the pair (%d, %d), which has no accumulator", sn, U[aq], U[bq]);
          want[acc] = {aq, bq};
        }
      size_t found = 0;
      for (int s = pl.rptr[sn]; s < pl.rptr[sn + 1]; ++s)
        for (int l = 0; l < 64; ++l) {
          const size_t q = (size_t)s * 64 + l;
          const bool chip = s < pl.rsplit[sn];
          const int tg = pl.rtgt[q], aq = pl.rab[q] & 0xFFFF, bq = (int)((unsigned)pl.rab[q] >> 16);
          if (tg == (chip ? g.accN : SCRATCH)) { CHECK(pl.rab[q] == 0, "rab", q, "padding slot"); continue; }
          int acc = tg;
          if (chip) {
            CHECK(tg >= 0 && tg < g.accN, "rtgt", q, "LDS offset %d outside the segment's %d accumulators", tg, g.accN);
            acc = tg < g.nL ? g.gL + tg : nnzL + g.c0 + (tg - g.nL);
          } else {
            CHECK(tg >= 0 && tg < nnzL + k, "rtgt", q, "accumulator %d out of range", tg);
            CHECK(!closedAcc[tg] , "rtgt", q, "HBM step updates accumulator %d of a closed segment", tg);
          }
          const auto it = want.find(acc);
          CHECK(it != want.end(), "rtgt", q, "accumulator %d is not updated by supernode %d (or occurs twice)", acc, sn);
          CHECK(it->second.first == aq && it->second.second == bq, "rab", q, "rows (%d, %d) of U, the accumulator %d belongs to (%d, %d)", aq, bq, acc, it->second.first, it->second.second);
          want.erase(it);
          ++found;
        }
      CHECK(want.empty(), "rtgt", (size_t)pl.rptr[sn] * 64, "supernode %d leaves %zu updated pairs out of its trailing schedule (first: accumulator %d)", sn, want.size(),
            want.empty() ? -1 : want.begin()->first);
      (void)found;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// (b) numeric emulation of qp_sparse.hip on the plan's schedules
struct Emu {
  dvec ACC, Dinv, x[2];
};

double kkt_value(const Entry &z, int kind, int idx, int r, int c)
{
  // kkt_fill, mode 0, no scaling (c = sx = sy = 1): the products with 1 change no bit
  if (kind == sfb::K_P) { double v = z.Px[idx]; if (r == c) v += kSigma; return v; }
  if (kind == sfb::K_A) return z.Ax[idx];
  if (kind == sfb::K_SIGMA) return kSigma;
  return -1.0 / kRho;
}

void emulate(const Entry &z, const SparsePlanHost &pl, const std::vector<SegV> &segs, Emu &E)
{
  const int k = pl.k, nnzL = pl.nnzL, pad = nnzL + k;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  E.ACC.assign((size_t)nnzL + k + 2, nan);
  E.Dinv.assign(k, nan);
  dvec &ACC = E.ACC;
  for (int zt = 0; zt < pl.nztop; ++zt)
    for (int p = 0; p < pl.ztop[2 * zt + 1]; ++p) {
      CHECK(pl.ztop[2 * zt] + p < (int)ACC.size(), "ztop", 2 * zt, "range leaves the workspace");
      ACC[pl.ztop[2 * zt] + p] = 0.0;
    }
  auto fill = [&](const ivec &desc, const ivec &map, int p0, int p1, dvec &dst, size_t bound, const char *nm) {
    for (int p = p0; p < p1; ++p) {
      CHECK(map[p] >= 0 && (size_t)map[p] < bound, nm, p, "fill target %d outside [0, %zu)", map[p], bound);
      dst[map[p]] = kkt_value(z, desc[4 * (size_t)p], desc[4 * (size_t)p + 1], desc[4 * (size_t)p + 2], desc[4 * (size_t)p + 3]);
    }
  };
  fill(pl.KdescT, pl.KmapT, 0, pl.nnzKT, ACC, ACC.size(), "KmapT");
  dvec t;
  const size_t LDS = (size_t)pl.lds_doubles;
  for (size_t si = 0; si < segs.size(); ++si) {
    const SegV &g = segs[si];
    t.assign(LDS, nan);
    if (pl.units) {
      // ldl_numeric_units: working set [own L | own D | outside | sink | zero | one]
      const int sink = g.accN + g.nout;
      CHECK((size_t)sink + 3 <= LDS, "seg", 12 * si + 6, "working set leaves the LDS");
      if (g.lds) {
        for (int e = 0; e < g.accN; ++e) t[e] = 0.0;
        fill(pl.Kdesc, pl.KmapL, g.kp0, g.kp1, t, g.accN, "KmapL");
      } else {
        for (int x = 0; x < g.accN; ++x) t[x] = ACC[x < g.nL ? g.gL + x : nnzL + g.c0 + (x - g.nL)];
      }
      for (int e = 0; e < g.nout; ++e) t[g.accN + e] = ACC[pl.uomap[g.omap0 + e]];
      t[sink] = 0.0; t[sink + 1] = 0.0; t[sink + 2] = 1.0;
      for (int u = g.a0; u < g.a1; ++u) {
        const bool dm = pl.ustream[(size_t)u * 256 + 1] == -1;  // (lane 0's second word)
        for (int h = 0; h < 2; ++h)
          for (int l = 0; l < 64; ++l) {
            const size_t q = (size_t)u * 256 + (size_t)l * 4 + 2 * h;
            const unsigned w0 = (unsigned)pl.ustream[q], w1 = (unsigned)pl.ustream[q + 1];
            const unsigned T = (w0 & 0xFFFFu) / 8, A = (w0 >> 16) / 8, B = (w1 & 0xFFFFu) / 8, D = (w1 >> 16) / 8;
            CHECK(T < LDS && A < LDS && (dm || (B < LDS && D < LDS)), "ustream", q, "offset outside the LDS");
            if (dm) t[T] = t[T] / t[A];
            else t[T] = std::fma(-t[A], t[B] * t[D], t[T]);
          }
      }
      for (int e = 0; e < g.nL; ++e) ACC[g.gL + e] = t[e];
      for (int j = g.c0; j < g.c1; ++j) {
        const double dd = t[g.nL + (j - g.c0)];
        CHECK(dd != 0.0, "D", j, "zero pivot");
        ACC[nnzL + j] = dd;
        E.Dinv[pl.f2s[j]] = 1.0 / dd;
      }
      for (int e = 0; e < g.nout; ++e) ACC[pl.uomap[g.omap0 + e]] = t[g.accN + e];
      continue;
    }
    // ldl_numeric_dev: supernodes of the segment, panels eliminated column by column, trailing slots in ascending member order
    double *scr = t.data();
    int gD = 0;
    if (g.lds) {
      CHECK((size_t)((g.accN + 3) & ~1) <= LDS, "seg", 12 * si + 6, "accumulators leave the LDS");
      for (int e = 0; e < g.accN + 2; ++e) t[e] = 0.0;
      fill(pl.Kdesc, pl.KmapL, g.kp0, g.kp1, t, g.accN, "KmapL");
      scr = t.data() + ((g.accN + 3) & ~1);
      gD  = nnzL + g.c0 - g.nL;
    }
    const size_t scratch = LDS - (size_t)(scr - t.data());
    dvec reg;
    for (int sn = g.a0; sn < g.a1; ++sn) {
      const int j0 = pl.snptr[sn], w = pl.snptr[sn + 1] - j0, R = pl.snR[sn];
      CHECK(w >= 1 && R >= w && (size_t)2 * w * R <= scratch, "snR", sn, "panel leaves the LDS scratch");
      double *pan = scr, *mul = scr + (size_t)w * R;
      const int32_t *pm = &pl.pmap[pl.poff[sn]], *pmL = &pl.pmapL[pl.poff[sn]];
      reg.assign((size_t)w * R, 0.0);
      for (int q = 0; q < w * R; ++q) {
        if (g.lds) { CHECK(pmL[q] >= 0 && pmL[q] < g.accN + 2, "pmapL", pl.poff[sn] + q, "offset outside the segment"); reg[q] = t[pmL[q]]; }
        else { CHECK(pm[q] >= 0 && pm[q] < pad + 2, "pmap", pl.poff[sn] + q, "accumulator out of range"); reg[q] = ACC[pm[q]]; }
      }
      for (int jj = 0; jj < w; ++jj) {
        const double dd = reg[(size_t)jj * R + jj];
        CHECK(dd != 0.0, "D", j0 + jj, "zero pivot");
        for (int r = jj; r < R; ++r) {
          const double v = reg[(size_t)jj * R + r] / dd;
          mul[(size_t)jj * R + r] = v * dd;
          if (r > jj) reg[(size_t)jj * R + r] = v;
          pan[(size_t)jj * R + r] = reg[(size_t)jj * R + r];
        }
        for (int rb = jj + 1; rb < w; ++rb)
          for (int ra = rb; ra < R; ++ra)
            reg[(size_t)rb * R + ra] = std::fma(-pan[(size_t)jj * R + ra], mul[(size_t)jj * R + rb], reg[(size_t)rb * R + ra]);
      }
      for (int jj = 0; jj < w; ++jj)
        for (int r = jj; r < R; ++r) {  // final values -> workspace (explicit zeros and the sink are skipped)
          const int q = jj * R + r;
          if (g.lds) {
            if (pmL[q] < g.accN) ACC[pmL[q] + (pmL[q] < g.nL ? g.gL : gD)] = reg[q];
            if (r == jj) t[pmL[q]] = reg[q];
          } else if (pm[q] < pad) ACC[pm[q]] = reg[q];
        }
      for (int jj = 0; jj < w; ++jj) E.Dinv[pl.f2s[j0 + jj]] = 1.0 / pan[(size_t)jj * R + jj];
      for (int s = pl.rptr[sn]; s < pl.rptr[sn + 1]; ++s)
        for (int l = 0; l < 64; ++l) {
          const size_t q = (size_t)s * 64 + l;
          const bool chip = s < pl.rsplit[sn];
          const int tg = pl.rtgt[q], a = w + (pl.rab[q] & 0xFFFF), b = w + (int)((unsigned)pl.rab[q] >> 16);
          CHECK(a < R && b < R, "rab", q, "row outside the panel");
          CHECK(tg >= 0 && (chip ? tg < g.accN + 2 : tg < pad + 2), "rtgt", q, "target out of range");
          double v = chip ? t[tg] : ACC[tg];
          for (int jj = 0; jj < w; ++jj) v = std::fma(-pan[(size_t)jj * R + a], mul[(size_t)jj * R + b], v);
          (chip ? t[tg] : ACC[tg]) = v;
        }
    }
  }
  // sweep copies, then forward sweep, 1 / D, backward sweep (ldl_sweep_copies, ldl_solve_dev)
  const int sc = pl.idx_scale;
  for (int rhs = 0; rhs < 2; ++rhs) {
    dvec w((size_t)k + 2, 0.0);
    for (int i = 0; i < k; ++i) w[i] = z.b[(size_t)rhs * k + pl.perm[i]];
    auto sweep = [&](const ivec &xmap, const ivec &xidx, int units) {
      for (int u = 0; u < units; ++u)
        for (int l = 0; l < 64; ++l)
          for (int s = 0; s < 2; ++s) {
            const size_t q = ((size_t)u * 64 + l) * 2 + s;
            const double Lv = xmap[q] >= 0 ? ACC[xmap[q]] : 0.0;
            const unsigned tg = ((unsigned)xidx[q] & 0xFFFFu) / sc, pv = ((unsigned)xidx[q] >> 16) / sc;
            CHECK(tg <= (unsigned)k && pv <= (unsigned)k, "xidx", q, "index outside the work vector");
            w[tg] = std::fma(-Lv, w[pv], w[tg]);
          }
    };
    sweep(pl.fmap, pl.fidx, pl.funits);
    for (int j = 0; j < k; ++j) w[j] = E.Dinv[j] * w[j];
    sweep(pl.bmap, pl.bidx, pl.bunits);
    E.x[rhs].assign(k, 0.0);
    for (int i = 0; i < k; ++i) E.x[rhs][pl.perm[i]] = w[i];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
void mutate(SparsePlanHost &pl, const std::string &what)
{
  if (what == "sweep") {  // swap two real slots of different steps of the forward sweep
    long first = -1, lastq = -1;
    for (size_t q = 0; q < pl.fmap.size(); ++q)
      if (pl.fmap[q] >= 0) { if (first < 0) first = (long)q; lastq = (long)q; }
    if (first < 0 || first / 128 == lastq / 128) { fprintf(stderr, "mutation sweep: the plan has a single step\n"); exit(3); }
    std::swap(pl.fmap[first], pl.fmap[lastq]);
    std::swap(pl.fidx[first], pl.fidx[lastq]);
  } else if (what == "ustream") {  // redirect one outside accumulator
    if (!pl.units) { fprintf(stderr, "mutation ustream: not a unit plan\n"); exit(3); }
    for (int s = 0; s < pl.nseg; ++s)
      if (pl.seg[12 * s + 10] >= 2) {
        int32_t *om = &pl.uomap[pl.seg[12 * s + 11]];
        om[0] = om[0] + 1 == om[1] ? om[0] + 2 : om[0] + 1;
        return;
      }
    fprintf(stderr, "mutation ustream: no segment with outside accumulators\n");
    exit(3);
  } else if (what == "supernodal") {  // exchange the row pair of one trailing slot with its neighbour's
    if (pl.units) { fprintf(stderr, "mutation supernodal: not a supernodal plan\n"); exit(3); }
    for (size_t q = 0; q + 1 < (size_t)pl.rsteps * 64; ++q)
      if (pl.rab[q] != pl.rab[q + 1] && pl.rab[q + 1] != 0 && q / 64 == (q + 1) / 64) { std::swap(pl.rab[q], pl.rab[q + 1]); return; }
    fprintf(stderr, "mutation supernodal: no two neighbouring trailing slots\n");
    exit(3);
  } else if (what == "kmap") {  // two KKT entries exchange their accumulators
    ivec &mp = pl.nnzKT >= 2 ? pl.KmapT : pl.KmapL;
    const int cnt = pl.nnzKT >= 2 ? pl.nnzKT : pl.nnzK;
    for (int p = 0; p + 1 < cnt; ++p)
      if (mp[p] != mp[p + 1]) { std::swap(mp[p], mp[p + 1]); return; }
    fprintf(stderr, "mutation kmap: nothing to exchange\n");
    exit(3);
  } else {
    fprintf(stderr, "unknown mutation %s\n", what.c_str());
    exit(3);
  }
}

struct Built { SparsePlanHost pl; Emu emu; };
Built g_default, g_supernodal, g_prev_default, g_prev_supernodal;  // (globals: nothing is left unreachable when a violation ends the run)

void run_plan(const Entry &z, const char *engine, const SparsePlanHost *prev, const std::string &mut, Built &out)
{
  g_where = z.name + "/" + engine;
  const int k = z.n + z.m;
  const char *msg = "";
  const int32_t *up = z.has_perm ? z.perm.data() : nullptr;
  int hint = 0;
  if (z.chain) {
    if (!prev) { fprintf(stderr, "%s: chained entry without a predecessor\n", z.name.c_str()); exit(2); }
    CHECK(prev->k == k, "perm", 0, "chained entry of another size");
    up = prev->perm.data();
    hint = prev->lds_doubles;
  }
  SparsePlanHost &pl = out.pl;
  const bool ok = sfb::build_sparse_plan(z.n, z.m, z.Pp.data(), z.Pi.data(), z.Ap.data(), z.Aj.data(), z.ordering, up,
                                         z.has_stage && !z.chain ? z.stage.data() : nullptr, pl, &msg, hint);
  CHECK(ok, "build_sparse_plan", 0, "refused: %s", msg);
  if (!mut.empty()) mutate(pl, mut);
  CHECK(pl.k == k && pl.n == z.n && pl.m == z.m, "k", 0, "sizes");
  CHECK(pl.idx_scale == (((k + 1) * 8 < (1 << 16)) ? 8 : 1), "idx_scale", 0, "%d for k = %d", pl.idx_scale, k);
  CHECK(pl.lds_doubles >= k + 2, "lds_doubles", 0, "%d < k + 2: the work vector of the sweeps does not fit", pl.lds_doubles);
  Derived d;
  derive(pl, d);
  Ref R;
  reference(z, pl.perm, pl.f2s, R);
  // the plan's pattern of L is the reference's own fill
  for (int j = 0; j < k; ++j) {
    CHECK(d.FLp[j + 1] - d.FLp[j] == (int)R.col[j].size(), "Lp", pl.f2s[j], "column %d of the factor numbering has %d entries, the fill of the reference %zu", j,
          d.FLp[j + 1] - d.FLp[j], R.col[j].size());
    for (size_t e = 0; e < R.col[j].size(); ++e) CHECK(d.FLi[d.FLp[j] + e] == R.col[j][e].first, "Li", d.FLp[j] + e, "row differs from the reference's fill");
  }
  // KKT column pointers in F (from the reference's side: entries per column of the permuted lower matrix)
  ivec FKp(k + 1, 0);
  {
    CHECK((int)pl.Kp.size() == k + 1, "Kp", 0, "size");
    for (int j = 0; j < k; ++j) FKp[j + 1] = FKp[j] + (pl.Kp[pl.f2s[j] + 1] - pl.Kp[pl.f2s[j]]);
  }
  const std::vector<SegV> segs = check_segments(pl, d, FKp);
  check_kmaps(z, pl, d, segs, FKp);
  check_sweep(pl, d, true);
  check_sweep(pl, d, false);
  if (pl.units) check_units(pl, d, segs);
  else check_supernodes(pl, d, segs);
  emulate(z, pl, segs, out.emu);
  const Emu &E = out.emu;
  for (int j = 0; j < k; ++j) {
    CHECK(E.ACC[pl.nnzL + j] == R.D[j], "D", j, "emulated %.17g, reference %.17g", E.ACC[pl.nnzL + j], R.D[j]);
    CHECK(E.ACC[pl.nnzL + j] != 0.0, "D", j, "zero pivot");
    CHECK(E.Dinv[pl.f2s[j]] == 1.0 / R.D[j], "Dinv", pl.f2s[j], "emulated %.17g", E.Dinv[pl.f2s[j]]);
    for (size_t e = 0; e < R.col[j].size(); ++e)
      CHECK(E.ACC[d.FLp[j] + e] == R.col[j][e].second, "L", d.FLp[j] + e, "entry (%d, %d): emulated %.17g, reference %.17g", R.col[j][e].first, j, E.ACC[d.FLp[j] + e],
            R.col[j][e].second);
  }
  for (int rhs = 0; rhs < 2; ++rhs)
    for (int i = 0; i < k; ++i)
      CHECK(E.x[rhs][i] == R.x[rhs][i], rhs ? "x1" : "x0", i, "solution: emulated %.17g, reference %.17g", E.x[rhs][i], R.x[rhs][i]);
  int closed = 0, maxR = 0;
  for (const SegV &g : segs) closed += g.lds;
  for (int r : pl.snR) maxR = std::max(maxR, r);
  printf("{\"name\": \"%s\", \"engine\": \"%s\", \"k\": %d, \"nnzL\": %d, \"units\": %d, \"lds_doubles\": %d, \"idx_scale\": %d, \"closed\": %d, \"open\": %d, "
         "\"nunits\": %d, \"nsn\": %d, \"maxcol\": %d, \"maxR\": %d, \"funits\": %d, \"bunits\": %d",
         z.name.c_str(), engine, k, pl.nnzL, pl.units, pl.lds_doubles, pl.idx_scale, closed, pl.nseg - closed, pl.nunits, pl.nsn, pl.maxcol, maxR, pl.funits, pl.bunits);
  if (k <= 400) {
    printf(", \"x\": [");
    for (int i = 0; i < k; ++i) printf("%s%.17g", i ? ", " : "", E.x[0][i]);
    printf("]");
  }
  printf("}\n");
  fflush(stdout);
}

}  // namespace

int main(int argc, char **argv)
{
  if (argc < 2) { fprintf(stderr, "usage: %s ZOOFILE [--only NAME] [--mutate sweep|ustream|supernodal|kmap]\n", argv[0]); return 2; }
  std::string only, mut;
  for (int a = 2; a + 1 < argc; a += 2) {
    if (!strcmp(argv[a], "--only")) only = argv[a + 1];
    else if (!strcmp(argv[a], "--mutate")) mut = argv[a + 1];
    else { fprintf(stderr, "unknown option %s\n", argv[a]); return 2; }
  }
  const std::vector<Entry> zoo = read_zoo(argv[1]);
  bool have_prev = false;
  for (const Entry &z : zoo) {
    if (!only.empty() && z.name != only && !(z.chain && have_prev)) { have_prev = false; continue; }
    Built &bd = g_default, &bs = g_supernodal;
    bd = Built();
    bs = Built();
    // the supernodal mutation applies to the SFB_PLAN_UNITS=0 plan, the unit-stream mutation to the default one
    sfb::knob_set("SFB_PLAN_UNITS", nullptr);
    run_plan(z, "default", z.chain ? &g_prev_default.pl : nullptr, mut == "supernodal" ? "" : mut, bd);
    sfb::knob_set("SFB_PLAN_UNITS", "0");
    run_plan(z, "supernodal", z.chain ? &g_prev_supernodal.pl : nullptr, mut == "ustream" ? "" : mut, bs);
    sfb::knob_set("SFB_PLAN_UNITS", nullptr);
    g_where = z.name + "/both engines";
    CHECK(bs.pl.units == 0, "units", 0, "SFB_PLAN_UNITS=0 did not select the supernodal engine");
    CHECK(bd.pl.perm == bs.pl.perm && bd.pl.f2s == bs.pl.f2s && bd.pl.nnzL == bs.pl.nnzL, "perm", 0, "the engines must share the orders");
    for (size_t e = 0; e < (size_t)bd.pl.nnzL + bd.pl.k; ++e)
      CHECK(bd.emu.ACC[e] == bs.emu.ACC[e], "ACC", e, "the engines differ: %.17g vs %.17g", bd.emu.ACC[e], bs.emu.ACC[e]);
    for (int rhs = 0; rhs < 2; ++rhs)
      for (int i = 0; i < bd.pl.k; ++i) CHECK(bd.emu.x[rhs][i] == bs.emu.x[rhs][i], "x", i, "the engines differ");
    std::swap(g_prev_default, bd);
    std::swap(g_prev_supernodal, bs);
    have_prev = true;
  }
  if (!mut.empty()) { fprintf(stderr, "mutation %s was NOT reported\n", mut.c_str()); return 4; }
  return 0;
}
