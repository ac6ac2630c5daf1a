// Forwarding header: reference include path and namespace for the functions over a collocation mesh
// (include/smooth_feedback_amd/mesh_function.hpp: MeshValue, mesh_eval, mesh_integrate, mesh_dyn).  `smooth::feedback` aliases `smooth_feedback_amd`.
#pragma once
#include "../../../smooth_feedback_amd/mesh_function.hpp"
namespace smooth { namespace feedback = ::smooth_feedback_amd; }
