// Prints the dense route table of csrc/qp_dense_route.h: one line "k time_limited big_off route" per combination.
// Stand-alone (own main, the header alone): tests/test_dense_route_host.py builds it with the sanitizers and runs it directly.
#include <cstdio>

#include "qp_dense_route.h"

static_assert(sfb::dense_route(32, false, false) == sfb::DenseRoute::Four, "usable in constant expressions");

static const char *name(sfb::DenseRoute r)
{
  switch (r) {
    case sfb::DenseRoute::Four: return "Four";
    case sfb::DenseRoute::Mid: return "Mid";
    case sfb::DenseRoute::Big: return "Big";
    case sfb::DenseRoute::FullPattern: return "FullPattern";
  }
  return "?";
}

int main()
{
  static const int ks[] = {1, 16, 17, 32, 33, 48, 64, 65, 128, 129, 1024, 1025, 19198};
  for (const int k : ks)
    for (int time_limited = 0; time_limited < 2; ++time_limited)
      for (int big_off = 0; big_off < 2; ++big_off)
        std::printf("%d %d %d %s\n", k, time_limited, big_off, name(sfb::dense_route(k, time_limited != 0, big_off != 0)));
  return 0;
}
