// The host flavour's replay entry points under AddressSanitizer + UBSan, as a stand-alone program (scripts/sanitize_cpu.sh builds it
// together with csrc/gobblet_cpu.cpp and runs it): a small synthetic window of 130 boards x 5 plies, about half of its cells valid,
// appended three times to rings of 37, 1 and 1 000 slots in exactly-sized heap blocks (with and without observations), and batches
// drawn from each.  Prints a checksum; any report of a sanitizer fails the run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../include/gobblet_cpu.h"

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

int main()
{
    const int64_t n = 130, stride = 192, cells = 5 * stride;
    const uint32_t plies = 5;
    uint32_t s = 7;
    std::vector<int8_t> obs(cells * 117), mask(cells * 54), z(cells), done(cells, 0), mover(cells);
    std::vector<int16_t> visits(cells * 54);
    for (auto &v : obs) v = (int8_t)(lcg(s) >> 31);
    for (auto &v : mask) v = (int8_t)(lcg(s) >> 31);
    for (auto &v : visits) v = (int16_t)(lcg(s) >> 28);
    for (auto &v : z) v = (lcg(s) >> 31) ? (int8_t)((int)(lcg(s) >> 30) % 3 - 1) : (int8_t)GBL_Z_OPEN;
    for (auto &v : mover) v = (int8_t)(lcg(s) >> 31);
    const size_t need = 32 + 16 * (plies - 1) * ((n + 63) / 64);  // gbl_replay_workspace_bytes (one function for both flavours)
    std::vector<uint8_t> ws(need);
    uint64_t sum = 0;
    for (int64_t capacity : {37, 1, 1000}) {
        for (int with_obs = 0; with_obs < 2; ++with_obs) {
            std::vector<int8_t> ring_obs(with_obs ? capacity * GBL_REPLAY_OBS_PITCH : 0), ring_meta(capacity * GBL_REPLAY_META_PITCH);
            std::vector<int16_t> ring_visits(capacity * GBL_REPLAY_VISITS_PITCH);
            uint64_t state[2] = {0, 0};
            for (int g = 0; g < 3; ++g) {
                const int rc = gbl_cpu_replay_append(with_obs ? obs.data() : nullptr, mask.data(), visits.data(), z.data(), done.data(), mover.data(), n,
                                                     plies, stride, 64, g, with_obs ? ring_obs.data() : nullptr, ring_visits.data(), ring_meta.data(),
                                                     capacity, state, ws.data(), need, nullptr);
                if (rc) { printf("append: %s\n", gbl_cpu_last_error()); return 1; }
            }
            for (int64_t recent : {0, 5}) {
                const int64_t batch = 200;
                std::vector<int8_t> o(batch * 117), m(batch * 54), zz(batch);
                std::vector<int16_t> v(batch * 54), sym(batch);
                std::vector<int32_t> index(2 * batch);
                const int rc = gbl_cpu_replay_batch(with_obs ? ring_obs.data() : nullptr, ring_visits.data(), ring_meta.data(), capacity, state, recent,
                                                    batch, 511, 3, 1, 2, with_obs ? o.data() : nullptr, m.data(), v.data(), zz.data(), index.data(),
                                                    sym.data(), nullptr);
                if (rc) { printf("batch: %s\n", gbl_cpu_last_error()); return 1; }
                for (int64_t j = 0; j < batch; ++j) sum += (uint64_t)index[2 * j] + (uint64_t)(uint16_t)v[j * 54] + (uint64_t)sym[j];
            }
            sum += state[0];
        }
    }
    printf("replay sanitize run: checksum %llu\n", (unsigned long long)sum);
    return 0;
}
