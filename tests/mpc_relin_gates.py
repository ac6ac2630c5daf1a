"""Shared by tests/test_mpc_relin_host.py and test_mpc_relin_gpu.py: the fixture tests/golden/mpc_relin_reference.npz
(tests/golden/make_golden_mpc_relin.py) and the gates of the re-linearisation passes.

Gate rule, as elsewhere in tests/: what a plain float64 numpy restatement (tests/mpc_relin_ref.py) differs by on the same inputs
is what float64 delivers there; a comparison is held to FOUR times that.  The row and Jacobian gates are re-measured inside
the host tests.  AUDIT_FACTOR is measured on the GPU, by test_mpc_relin_gpu.py::test_the_audit_falls_as_in_the_restatement, which
prints it: the worst ratio, over the fixture's agents and passes 0, 1, 2, of the dynamics error of the HOST path
(MPC::operator() with MPCParams::relin_passes) to the restatement's.  The restatement solves with the CPU oracle from its natural
elimination order and differences its Jacobians, but both polish their solutions, so the plans agree far below the size of the
audited errors (1e-1 .. 3e-5): the ratio measures 1.0000 to the four decimals the test prints, recorded here rounded up."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpc_relin_reference.npz")
MARGIN = 4.0
VARIANT = 6
KEPT = (0, 4, 5)
# worst host-path / restatement ratio of agent_max over agents and passes, as measured on the MI355X
AUDIT_FACTOR_MEASURED = 1.0001
# the existing gates the GPU tests reuse
U_TOL = 1e-6        # tests/test_mpc_devlin_gpu.py: device-linearised against host-linearised swarm
REC_TOL = 1e-12     # tests/test_mpc_devlin_gpu.py: kernel records against MPC::fill_record
PRUNED_TOL = 1e-6   # tests/test_mpc_gpu.py: a pruned plan against a plan of the whole pattern with another summation order
QP_EPS = 1e-3       # QPSolverParams: eps_abs = eps_rel of the MPC's default solver parameters


def fixture():
    fx = np.load(FIXTURE)
    return dict(K=int(fx["K"]), tf=float(fx["tf"]), t=fx["t"], dx0=fx["dx0"], agent_max=fx["agent_max"], code=fx["code"])


def audit_factor():
    assert AUDIT_FACTOR_MEASURED is not None, "AUDIT_FACTOR_MEASURED has not been measured"
    return MARGIN * AUDIT_FACTOR_MEASURED
