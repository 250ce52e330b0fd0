// Launch heuristics shared by the kernel files of the extension, so that two
// translation units that tile channels-last rows the same way cannot drift.
#pragma once

#include <cstdint>

namespace msbn {

// blocks a two-stage reduction aims for: 256 CUs x 8 blocks (guide G11)
constexpr int kTargetBlocks = 2048;

// Lanes of a 256-thread block laid across one channels-last row (each lane
// owns V consecutive channels); the other 256 / lpr thread rows walk the
// rows.  A power of two in [8, 256].  Defined in bn_kernels.hip.
int nhwc_lanes_per_row(int64_t C, int V);

}  // namespace msbn
