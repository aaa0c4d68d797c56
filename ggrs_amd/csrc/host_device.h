// host_device.h -- the few sizes that plain host code (p2p_plan.h and the test program built around
// it with a host compiler) shares with the kernels.  No HIP runtime header here.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define GGRS_HD __host__ __device__
#else
#define GGRS_HD
#endif

namespace ggrs {

constexpr int kWave = 64;

// u32 fields of a P-player state: frame + (x, y, vx, vy, rot) per player
GGRS_HD constexpr int state_fields(int p) { return 1 + 5 * p; }
// bytes of one session's input record: the players' bytes padded to a power of two
GGRS_HD constexpr int padded_players(int p) { return p <= 1 ? 1 : (p == 2 ? 2 : 4); }
GGRS_HD constexpr int64_t grid_of(int64_t n, int64_t block) { return (n + block - 1) / block; }

}  // namespace ggrs
