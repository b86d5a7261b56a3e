// blockers_dev.hpp — the launch of sr_blockers_plan's kernel (blockers.hip), for query.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "blockers.hpp"

namespace sr {

// Every candidate of `b` planned by a wave of its own; b.counts (when wanted) was zeroed on the stream.
hipError_t launch_blockers(const BlockersArgs& b, hipStream_t s);

}  // namespace sr
