// The host flavour's gbl_cpu_train_step_weighted and gbl_cpu_replay_importance under AddressSanitizer + UBSan, as a stand-alone program
// (its own main; nothing of it is loaded into python):
//   g++ -O1 -g -std=c++17 -mpopcnt -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined \
//       -Wno-unknown-pragmas -Wno-attributes -pthread -o /tmp/train_weighted_main scripts/sanitize_train_weighted_main.cpp \
//       gobblet-rl_amd/csrc/gobblet_cpu.cpp && /tmp/train_weighted_main
// Weighted steps at B in {1, 3, 65, 130} x H in {64, 256} with and without a mask, weights NULL and given (a 0, a denormal, -1, NaN and
// +inf among them), each of the two per-row outputs NULL in turn, priority maps at the floor, past 2^30 and with floor = cap; then
// importance weights at batch 1, 63, 64, 65 and 4 097 -- every array an exactly-sized heap block, the workspace exactly
// gbl_train_workspace_bytes.  Prints a checksum; any report of a sanitizer fails the run.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/gobblet_cpu.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static float unit(uint32_t &s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

int main()
{
    uint32_t s = 11;
    double sum = 0.0;
    for (int64_t B : {1, 3, 65, 130})
        for (int H : {64, 256}) {
            const size_t P = 173 * (size_t)H + 55, need = 4 * (size_t)B * (2 * (size_t)H + 60);  // gbl_train_workspace_bytes
            std::vector<int8_t> obs(B * 117), mask(B * 54), z(B);
            std::vector<int16_t> visits(B * 54);
            std::vector<float> params(P), m(P, 0.0f), v(P, 0.0f), grad(P), stats(4), weight(B), row_loss(2 * B);
            std::vector<int32_t> prio(B);
            std::vector<uint8_t> ws(need);
            for (auto &x : obs) x = (int8_t)(lcg(s) >> 29 == 0);
            for (auto &x : mask) x = (int8_t)(lcg(s) >> 31);
            for (int64_t r = 0; r < B; ++r) mask[r * 54 + (lcg(s) >> 16) % 54] = 1;
            for (auto &x : visits) x = (int16_t)(lcg(s) >> 25);
            for (auto &x : z) x = (int8_t)((int)(lcg(s) >> 30) % 3 - 1);
            if (B >= 3) z[1] = (int8_t)GBL_Z_OPEN;
            for (auto &x : params) x = (unit(s) - 0.5f) * 0.25f;
            for (auto &x : weight) x = 4.0f * (1.0f - unit(s));
            if (B >= 65) { weight[0] = 0.0f; weight[3] = 1e-41f; weight[4] = -1.0f; weight[5] = NAN; weight[7] = INFINITY; }
            int t = 0;
            for (int with_mask : {1, 0})
                for (int form = 0; form < 5; ++form) {
                    ++t;
                    const gbl_train_hyper hy{2e-3f, 0.9f, 0.999f, 1e-8f, 1e-4f, 1e-2f, (float)(1.0 - pow(0.9, t)), (float)(1.0 - pow(0.999, t))};
                    const float scale = form == 1 ? 0.0f : form == 2 ? 1e30f : 1000.0f;
                    const int32_t floor = form == 3 ? 5 : 1, cap = form == 3 ? 5 : 100000;
                    const int rc = gbl_cpu_train_step_weighted(obs.data(), with_mask ? mask.data() : nullptr, visits.data(), z.data(), B, H,
                                                               params.data(), m.data(), v.data(), &hy, form == 4 ? nullptr : weight.data(),
                                                               form == 1 ? nullptr : row_loss.data(), form == 2 ? nullptr : prio.data(), scale,
                                                               floor, cap, form == 0 ? nullptr : grad.data(), stats.data(), ws.data(),
                                                               (int64_t)need, nullptr);
                    if (rc) { printf("train_step_weighted: %s\n", gbl_cpu_last_error()); return 1; }
                    for (float x : stats) sum += x;
                    if (form != 2) for (int32_t x : prio) sum += x;
                    if (form != 1) for (float x : row_loss) sum += x;
                }
            for (float x : params) sum += x;
        }
    for (int64_t n : {1, 63, 64, 65, 4097}) {
        std::vector<int32_t> prio(n);
        std::vector<float> w(n);
        for (float beta : {0.0f, 0.4f, 1.0f})
            for (int dead = 0; dead < 2; ++dead) {
                for (auto &x : prio) x = dead ? -(int32_t)(lcg(s) >> 1) : (int32_t)(lcg(s) >> (1 + (lcg(s) >> 28))) - 3;
                if (!dead) prio[n / 2] = INT32_MAX;
                const int rc = gbl_cpu_replay_importance(prio.data(), n, beta, w.data(), nullptr);
                if (rc) { printf("replay_importance: %s\n", gbl_cpu_last_error()); return 1; }
                for (float x : w) sum += x;
            }
    }
    if (!(sum == sum)) { printf("the checksum is not a number\n"); return 1; }
    printf("train_weighted sanitize checksum %.6f\n", sum);
    return 0;
}
