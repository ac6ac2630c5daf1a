"""smooth_feedback_amd: MI355X-native batched QP / MPC / EKF engine behind the smooth::feedback API.

The compute path is libsfb.so (hand-written HIP for gfx950, C-ABI in include/sfb.h).  This package
is the thin host-side mirror of the reference interface used by tests and bench.py.
"""
from . import _capi  # noqa: F401  (fails loudly if libsfb.so is missing)
from ._capi import debug_set, debug_set_from  # noqa: F401  (debug knobs of the library: tests, A/B measurements)
from .qp import (QPBatchSolution, QPSolution, QPSolutionStatus, QPSolver, QPSolverParams,  # noqa: F401
                 QuadraticProgram, pack_colmajor, random_qp_batch, solve_qp, solve_qp_batch_device, solve_qp_batch_device_phases,
                 solve_qp_batch_device_trace, solve_qp_batch_device_ws, Workspace,
                 solve_qp_batch_host, QuadraticProgramSparse, SparseQPPlan, solve_qp_sparse,
                 solve_qp_tall_batch_device, solve_qp_tall_batch_host)

from .ekf import (ekf_predict_batch_device, ekf_predict_batch_host, ekf_predict_rk4_batch_device, ekf_predict_stepper_batch_device,  # noqa: F401
                  ekf_predict_update_batch_device, ekf_step_batch_host, ekf_update_batch_device)
from .pid import (PIDGroup, pid_rollout_batch_device, pid_rollout_batch_host, pid_rollout_spline_batch_device,  # noqa: F401
                  pid_rollout_spline_batch_host,
                  pid_step_batch_device, pid_step_batch_host)
from .spline import (spline_eval_batch_device, spline_eval_batch_host, spline_fit_cubic_batch_device,  # noqa: F401
                     spline_fit_cubic_batch_host)
from .mesh import (PHMesh, mesh_dyn_batch, mesh_dyn_batch_device, mesh_dyn_batch_host, mesh_dyn_error_batch_device,  # noqa: F401
                   mesh_dyn_error_batch_host, mesh_dyn_pattern, mesh_eval_batch, mesh_eval_batch_device, mesh_eval_batch_host,
                   mesh_eval_pattern, mesh_integrate_batch, mesh_integrate_batch_device, mesh_integrate_batch_host,
                   mesh_resample_batch_device, mesh_resample_batch_host, ocp_nlp_batch, ocp_nlp_batch_device, ocp_nlp_batch_host,
                   ocp_nlp_bounds, ocp_nlp_hess_batch, ocp_nlp_hess_batch_device, ocp_nlp_hess_batch_host, ocp_nlp_hess_pattern, ocp_nlp_pattern,
                   ocp_nlp_structure)
from .nlp import NLPSQPParams, NLPSwarmSQP, NLPSwarmSolution, nlp_sqp_qp_pattern  # noqa: F401
from .mpc import LIE_RN, LIE_SE2, LIE_SE3, LIE_SO3, MPCLayout, MPCSwarm  # noqa: F401

__version__ = "0.1.0"
