// explain_dev.hpp — launches of the explain and shortfall kernels (explain.hip, explain_plan.hip), shared with
// query.cpp.  Their arguments are explain_args.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include "explain_args.hpp"
#include "node_view.hpp"

namespace sr {

hipError_t launch_explain(const ExplainArgs& a, hipStream_t s);
hipError_t launch_explain_plan(const ExplainPlanArgs& a, hipStream_t s);

hipError_t launch_shortfall(const ExplainArgs& a, const ShortfallArgs& sa, hipStream_t s);
// (pa.node_slack is not read: the slack is node_left clamped)
hipError_t launch_shortfall_plan(const ExplainPlanArgs& pa, const ShortfallArgs& sa, hipStream_t s);
// closes the partials of every query (after the launches above, on the same stream)
hipError_t launch_shortfall_close(int32_t n_pods, const ShortfallArgs& sa, hipStream_t s);

// sr_node_view_pods / sr_node_view_plan (node_view.hip): every active query of `pa` folded per node into the
// partials, then the partials into the call's totals, on the same stream.  pa.x.sums / node_mask and
// pa.node_slack are not read or written.
hipError_t launch_node_view(const ExplainPlanArgs& pa, const NodeViewArgs& na, hipStream_t s);

}  // namespace sr
