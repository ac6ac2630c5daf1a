// Forwarding header: reference include path and namespace for the collocation NLP front
// (include/smooth_feedback_amd/ocp_to_nlp.hpp: ocp_to_nlp, nlpsol_to_ocpsol, ocpsol_to_nlpsol).  `smooth::feedback` aliases `smooth_feedback_amd`.
#pragma once
#include "../../smooth_feedback_amd/ocp_to_nlp.hpp"
namespace smooth { namespace feedback = ::smooth_feedback_amd; }
