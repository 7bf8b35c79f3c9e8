// net_consts.hpp — the constants shared by the device code (forward_common.hpp), the layouts
// (image_layout.hpp) and the HIP-free host code (params_host.hpp).
#pragma once

namespace mib {

constexpr int F2 = 16;          // filters (F1 == F2, D == 1)
constexpr int N_OUT = 4;        // classes
constexpr int FMAGIC_I = 0x4B400000;   // bit pattern of 1.5 * 2^23

}  // namespace mib
