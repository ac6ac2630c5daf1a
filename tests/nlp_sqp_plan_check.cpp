// Stand-alone run of the swarm SQP pattern builder (csrc/nlp_sqp_plan.cpp): host code only, its own main.  Built by
// tests/test_nlp_sqp_host.py from this file and nlp_sqp_plan.cpp with AddressSanitizer and UBSan -- no HIP, no libsfb.so.
//
//   nlp_sqp_plan_check ZOOFILE
//
// ZOOFILE is text: the number of entries, then per entry  name n m nnzJ nnzH | J_rowptr | J_colind | H_colptr | H_rowind |
// xl | xu | gl | gu  (strtod spells the infinities and NaN).  Per entry one JSON line goes to stdout: {"name", "ok", "msg",
// "nb", and every array of the pattern}.  The caller compares them with its own restatement.
#include "../smooth_feedback_amd/csrc/nlp_sqp_plan.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

namespace {

std::vector<int32_t> ints(std::istream &in, int count)
{
  std::vector<int32_t> v((size_t)count);
  for (auto &x : v) in >> x;
  return v;
}

std::vector<double> doubles(std::istream &in, int count)
{
  std::vector<double> v((size_t)count);
  std::string tok;
  for (auto &x : v) {
    in >> tok;
    x = std::strtod(tok.c_str(), nullptr);
  }
  return v;
}

void put(const char *key, const std::vector<int32_t> &v)
{
  std::printf(", \"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf(i ? ", %d" : "%d", v[i]);
  std::printf("]");
}

}  // namespace

int main(int argc, char **argv)
{
  if (argc != 2) {
    std::fprintf(stderr, "usage: nlp_sqp_plan_check ZOOFILE\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  int entries = 0;
  if (!(in >> entries)) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  for (int e = 0; e < entries; ++e) {
    std::string name;
    int n = 0, m = 0, nnzJ = 0, nnzH = 0;
    in >> name >> n >> m >> nnzJ >> nnzH;
    // every array in a buffer of exactly its length: an index the builder should not touch is a finding of the sanitizer
    const auto Jp = ints(in, m + 1), Jj = ints(in, nnzJ), Hp = ints(in, n + 1), Hi = ints(in, nnzH);
    const auto xl = doubles(in, n), xu = doubles(in, n), gl = doubles(in, m), gu = doubles(in, m);
    if (!in) {
      std::fprintf(stderr, "entry %d of %s is cut short\n", e, argv[1]);
      return 2;
    }
    sfb::NlpSqpPattern o;
    const char *msg = "";
    const bool ok   = sfb::build_nlp_sqp_pattern(n, m, Jp.data(), Jj.data(), Hp.data(), Hi.data(), xl.data(), xu.data(), gl.data(), gu.data(), o, &msg);
    std::printf("{\"name\": \"%s\", \"ok\": %s, \"msg\": \"%s\", \"nb\": %d", name.c_str(), ok ? "true" : "false", msg, o.nb);
    if (ok) {
      put("A_rowptr", o.A_rowptr); put("A_colind", o.A_colind); put("P_colptr", o.P_colptr); put("P_rowind", o.P_rowind);
      put("P_src", o.P_src); put("P_diag", o.P_diag); put("Jc_colptr", o.Jc_colptr); put("Jc_row", o.Jc_row); put("Jc_pos", o.Jc_pos);
      put("bound_var", o.bound_var); put("bound_row", o.bound_row);
    }
    std::printf("}\n");
  }
  return 0;
}
