// Constants of the device sampler that the kernels (nxc_kernels.hpp) and the host-only descriptor
// checks (nxc_desc_check.hpp) share: plain C++, no device code.
#pragma once
#include <cstdint>

// NumPy's PCG64 on the device (PcgK): affine maps of 2^b steps and of the start of draw vector v
constexpr int NXC_PCG_BITS = 40, NXC_PCG_VECS = 8;    // rows below 2^40; draws per packet
// Rejection trials per packet of a surface spot: the host sizes the budget to the map (32 /
// acceptance rate, so that a packet fails to find a launch point with probability e^-32) between
// these bounds; a packet that never passes is reported, and the call fails.
constexpr int NXC_SPOT_MIN_TRIALS = 4096, NXC_SPOT_MAX_TRIALS = 1 << 18;
constexpr int64_t NXC_NODE_TABLE_MAX = 1 << 16;       // entries per row of a per-node table
// which k_sample instantiation a source runs (nxc_kernels.hpp)
constexpr int NXC_LAW_PLAIN = 0, NXC_LAW_THERMAL = 1, NXC_LAW_NODES = 2;
