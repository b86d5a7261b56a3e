// evacuate_dev.hpp — the launch of sr_evacuate_plan's kernel (evacuate.hip), for query.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "evacuate.hpp"

namespace sr {

// Every scenario of `b` planned by a block of b.waves waves, `blocks` blocks taking them grid-stride; b.counts
// (when wanted) was zeroed on the stream, and the scratch behind b.used / b.added (evacuate_scratch(n_pad,
// blocks)) is zero before the launch and zero again after it.
hipError_t launch_evacuate(const EvacuateArgs& b, int32_t blocks, hipStream_t s);

}  // namespace sr
