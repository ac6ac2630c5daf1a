// Forwarding header: reference include path and namespace for solve_nlp_sqp, the NLP solver of this repository
// (include/smooth_feedback_amd/nlp_solver.hpp; it stands where the reference has compat/ipopt.hpp's solve_nlp_ipopt).
// `smooth::feedback` aliases `smooth_feedback_amd`.
#pragma once
#include "../../smooth_feedback_amd/nlp_solver.hpp"
namespace smooth { namespace feedback = ::smooth_feedback_amd; }
