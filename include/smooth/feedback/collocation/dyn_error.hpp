// Forwarding header: reference include path and namespace for the collocation dynamics-error estimate
// (include/smooth_feedback_amd/dyn_error.hpp: mesh_dyn_error, flat_dynamics).  `smooth::feedback` aliases `smooth_feedback_amd`.
#pragma once
#include "../../../smooth_feedback_amd/dyn_error.hpp"
namespace smooth { namespace feedback = ::smooth_feedback_amd; }
