// Dense QP path: which kernel takes a batch of k = n + m.  Plain C++ (no HIP, no sfb.h): a host compiler builds it alone.
//
//   k <= 32, no time limit   Four         qp_dense4.hip     four QPs per wavefront (one per 16-lane row), factor in VGPRs
//   otherwise k <= 128       Mid          qp_dense_mid.hip  one QP per wavefront, everything on chip: registers-only engine
//                                                           up to 64, LDS block engine beyond
//   otherwise k <= 1024      Big          qp_dense_big.hip  one QP per wavefront, pivoted LDL' with the factor in HBM
//   otherwise                FullPattern  qp_sparse.hip     the shared-pattern sparse kernel on a full pattern, no pivoting
//
//   A time limit (QPSolverParams::max_time, qp_solver.hpp:504-507) on k <= 32 goes to Mid, whose smallest instance serves
//   every k <= 48 and compares the wall clock at every stopping check that leaves the status open; the four-per-wave
//   kernel time-slices its slots and carries no per-QP clock.
//   SFB_QP_DENSE_BIG=0 (A/B, tests) turns Big off: those sizes take FullPattern as well.  It does not move k <= 128.
// Four, Mid and Big are bit-identical to oracle/qp_oracle.c, so the routing among them never shows in a result;
// FullPattern factorises in another order and agrees to rounding.
#pragma once

namespace sfb {

enum class DenseRoute { Four, Mid, Big, FullPattern };

constexpr int kDenseFourMaxK = 32;
constexpr int kDenseMidMaxK  = 128;
constexpr int kDenseBigMaxK  = 1024;

constexpr DenseRoute dense_route(int k, bool time_limited, bool big_off)
{
  if (k <= kDenseFourMaxK && !time_limited) return DenseRoute::Four;
  if (k <= kDenseMidMaxK) return DenseRoute::Mid;
  if (k <= kDenseBigMaxK && !big_off) return DenseRoute::Big;
  return DenseRoute::FullPattern;
}

}  // namespace sfb
