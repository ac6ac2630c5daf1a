// Forwarding header: reference include path and namespace for the flattening of Lie-group problems
// (include/smooth_feedback_amd/ocp_flatten.hpp: flatten_ocp, FlatHess, unflatten_ocpsol).  `smooth::feedback` aliases `smooth_feedback_amd`.
#pragma once
#include "../../smooth_feedback_amd/ocp_flatten.hpp"
namespace smooth { namespace feedback = ::smooth_feedback_amd; }
