// Forwarding header: reference include path and namespace for the ph collocation mesh
// (include/smooth_feedback_amd/mesh.hpp: Mesh<Kmin, Kmax>).  `smooth::feedback` aliases `smooth_feedback_amd`.
#pragma once
#include "../../../smooth_feedback_amd/mesh.hpp"
namespace smooth { namespace feedback = ::smooth_feedback_amd; }
