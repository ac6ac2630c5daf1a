// Forwarding header: reference include path and namespace for the NLP concepts and NLPSolution
// (include/smooth_feedback_amd/nlp.hpp).  `smooth::feedback` aliases `smooth_feedback_amd`.
#pragma once
#include "../../smooth_feedback_amd/nlp.hpp"
namespace smooth { namespace feedback = ::smooth_feedback_amd; }
