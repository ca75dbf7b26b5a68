// train_math.cpp -- TEST INFRASTRUCTURE: gobblet-rl_amd/csrc/gobblet_device.h compiled for the host (as gobblet_cpu.cpp compiles it, with
// the host flavour's flags) so that tests/test_train_step.py can run the library's OWN train_exp and train_log, array in / array out,
// over a dense grid.  Built by the test into a temporary directory; nothing of the product includes it.
#define GBL_HOST_EMU
#include <stdint.h>
#include <string.h>

#define __device__
#define __forceinline__ inline
struct uint4 {
    uint32_t x, y, z, w;
};
static inline uint32_t host_alignbyte(uint32_t hi, uint32_t lo, uint32_t n) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (n & 3u))); }
static inline uint32_t host_udot4(uint32_t a, uint32_t b, uint32_t c, bool)
{
    for (int i = 0; i < 4; ++i) c += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
    return c;
}
static inline uint32_t host_umul24(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)(a & 0xFFFFFFu) * (b & 0xFFFFFFu)); }
static inline uint32_t host_umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
#define __builtin_amdgcn_alignbyte host_alignbyte
#define __builtin_amdgcn_udot4 host_udot4
#define __umul24 host_umul24
#define __umulhi host_umulhi
#define __popc __builtin_popcount
#define __popcll __builtin_popcountll
#define __shfl_down(v, delta) (0u)

#include "../../gobblet-rl_amd/csrc/gobblet_device.h"

extern "C" {
void train_math_exp(const float *x, float *out, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) out[i] = gbl::train_exp(x[i]);
}
void train_math_log(const float *s, float *out, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) out[i] = gbl::train_log(s[i]);
}
}
