"""Gates of the swarm SQP tests, each with the measurement it comes from.  The measurements are the CPU reference's
(tests/nlp_sqp_ref.py: the law in numpy float64, QPs by the CPU oracle's dense solver at eps_abs = eps_rel = 1e-9, polished),
never the code under test's; tests/test_nlp_sqp_host.py::test_reference_law_solves_hs71_from_every_start re-measures them and
fails when they move.

HS71, the standard start (1, 5, 5, 1) and 24 seeded starts within 0.1 / 0.3 of it (nlp_sqp_ref.hs71_starts), reference run
with tol = 1e-7 and a cap of 40 iterations:
  every start ends Optimal with |f - 17.0140173| <= 1.1e-8;
  iterations: 8 for 23 starts, 6 for two; QP solves: 15 resp. 12 (the first iteration climbs the ladder to mu = 26.2 resp. 3.28);
  largest final residuals over the starts: stationarity 1.36e-8, violation 1.71e-10, complementarity 8.9e-21.
The residuals fall quadratically (1e-5, 1e-8, 1e-12 over the last iterations, the polished QP being exact to rounding), so a
final residual is whatever the first iterate below the reference's tol happened to have.
"""
GATE_FACTOR = 4.0                     # the project's factor between a measurement and its gate

HS71_REF_TOL = 1e-7                   # the tolerance the reference ran with
HS71_REF_CAP = 40
HS71_WORST_RESIDUAL = 1.36e-8         # measured: the largest final residual of the 25 reference runs (stationarity, start 16)
HS71_MAX_ITER = 8                     # measured: the largest iteration count of the 25 reference runs
HS71_F_TOL = 1e-6                     # the issue's: |f - 17.0140173|

HS71_GPU_TOL = GATE_FACTOR * HS71_WORST_RESIDUAL
HS71_GPU_CAP = HS71_MAX_ITER + 2      # the GPU's sparse QP solve differs from the dense oracle's in elimination order

# The reference's Ipopt-test problem with tf pinned to 5 (nlp_sqp_ref.ocp_problem: double integrator, two intervals of degree 4,
# n = 28, 30 + 1 QP rows), from the straight line and two seeded perturbations of it (nlp_sqp_ref.ocp_starts); gates as for HS71:
# reference run with tol = 1e-7 and a cap of 40 iterations.
#   the perturbed starts end Optimal after 5 and 7 iterations (7 and 9 QP solves) with residuals 2.7e-15 and 3.7e-15;
#   the straight line takes four full steps to violation 7e-16 and stationarity 5.8e-5 and then CRAWLS: the objective is the
#   variable q, tied to the states by the integral row, and the l1 merit rejects the full step near the solution (the Maratos
#   effect; a second-order correction is out of this solver's scope), alpha falls to 1/8 .. 1/32 and stationarity goes 2.9e-5,
#   2.2e-5, 1.1e-5, 9.5e-6 ... 3.68e-7, 3.453e-7 at the cap: MaxIterations, final residual 3.453e-7 (violation 5.7e-16).
#   objective 7.1619072446 at all three ends.
# So the largest final residual the reference recorded is 3.453e-7 and its largest count 40.
OCP_WORST_RESIDUAL = 3.46e-7          # measured: the largest final residual of the three reference runs (stationarity, start 0)
OCP_MAX_ITER = 40                     # measured (the cap: start 0)
OCP_OBJECTIVE = 7.1619072446          # measured: q at the reference's three ends
OCP_GPU_TOL = GATE_FACTOR * OCP_WORST_RESIDUAL
OCP_GPU_CAP = OCP_MAX_ITER + 2

# The reference's own scenario, tf in [3, 6], same mesh, from the straight line with tf = 5: the reference law ends Optimal after
# 18 iterations and 34 QP solves (the ladder works on most iterations, mu up to 0.1), tf at its bound 6, objective 7.06262428,
# final residuals: stationarity 2.843e-8, violation 1.07e-13, complementarity 9e-25; the last iterations take full steps
# (1.4e-6, 1.5e-7, 2.8e-8).  From tf = 4 it arrives as well (29 iterations), so the scenario is gated on the GPU.
OCP_FREE_WORST_RESIDUAL = 2.85e-8     # measured
OCP_FREE_MAX_ITER = 18                # measured
OCP_FREE_OBJECTIVE = 7.06262428       # measured
OCP_FREE_TF = 6.0
OCP_FREE_GPU_TOL = GATE_FACTOR * OCP_FREE_WORST_RESIDUAL
OCP_FREE_GPU_CAP = OCP_FREE_MAX_ITER + 2
OCP_OBJECTIVE_TOL = 1e-6              # as HS71's |f - f*|: both ends are feasible to 1e-12 and stationary to the gates above
