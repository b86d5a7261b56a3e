// launch_shape.hpp — the shape of a K2 launch, decided from plain scalars.
// No HIP in here: the launchers (kernels.hip), the planner (planner.cpp) and
// the residency unit (residency.cpp) all take these rules from this one place.
#pragma once

#include <cstdint>

namespace sr {

constexpr int32_t kNodeKernelMaxPods = 4 * 64;  // the node-order kernel plans up to four groups of 64 pods
constexpr int32_t kWideListMax = 2048;          // longest list that runs one wave per block

// The launch takes the node-order kernel: no candidate on the domain path,
// node order allowed (SR_K2_MODE=0), every candidate within the kernel's pod
// count, and the kernel switched on (SR_K2_NODE_KERNEL).
inline bool k2_node_launch(bool domain_path, int32_t k2_mode, int32_t max_np, int32_t node_kernel) {
  return !domain_path && k2_mode == 0 && max_np >= 1 && max_np <= kNodeKernelMaxPods && node_kernel != 0;
}

// Groups of 64 pods the node-order kernel is instantiated for (1, 2 or 4).
inline int k2_node_groups(int32_t max_np) { return max_np <= 64 ? 1 : (max_np <= 128 ? 2 : 4); }

// K2 waves per block: SR_K2_WPB (1, 2, 4), else one wave per block for lists of
// at most 2,048 entries (the waves spread over every CU, so a long chain wave
// shares its CU with fewer others: C5 K2 38.2 -> 36.1 us, realistic C3 31.5 ->
// 30.5, C3 15.0 -> 14.4) and four above (C4: 15,000 waves)
inline int k2_waves_per_block(int32_t wpb_switch, int32_t n_list) {
  if (wpb_switch == 1 || wpb_switch == 2 || wpb_switch == 4) return wpb_switch;
  return n_list <= kWideListMax ? 1 : 4;
}

}  // namespace sr
