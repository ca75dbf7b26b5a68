// The host flavour's prioritised-replay entry points under AddressSanitizer + UBSan, as a stand-alone program (scripts/sanitize_cpu.sh
// builds it together with csrc/gobblet_cpu.cpp and runs it): scripts/sanitize_replay_main.cpp's synthetic window appended three times to
// rings of 37, 1, 33 and 1 000 slots with gbl_cpu_replay_prio_append behind every append (a scalar, then a per-cell array), the index
// built, batches drawn and the drawn rows' priorities updated -- ring_prio, the index and every output in exactly-sized heap blocks.
// Prints a checksum; any report of a sanitizer fails the run.
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
    std::vector<int32_t> prio_traj(cells);
    for (auto &v : obs) v = (int8_t)(lcg(s) >> 31);
    for (auto &v : mask) v = (int8_t)(lcg(s) >> 31);
    for (auto &v : visits) v = (int16_t)(lcg(s) >> 28);
    for (auto &v : z) v = (lcg(s) >> 31) ? (int8_t)((int)(lcg(s) >> 30) % 3 - 1) : (int8_t)GBL_Z_OPEN;
    for (auto &v : mover) v = (int8_t)(lcg(s) >> 31);
    for (auto &v : prio_traj) v = (int32_t)(lcg(s) >> 20) - 1000;  // (about a quarter negative: weight 0)
    const size_t need = 32 + 16 * (plies - 1) * ((n + 63) / 64);  // gbl_replay_workspace_bytes (one function for both flavours)
    std::vector<uint8_t> ws(need);
    uint64_t sum = 0;
    for (int64_t capacity : {37, 1, 33, 1000}) {
        const size_t leaves = (capacity + 31) / 32, index_bytes = 8 * (2 + (leaves + 63) / 64 + 1 + leaves);  // gbl_replay_prio_index_bytes (likewise)
        std::vector<int8_t> ring_obs(capacity * GBL_REPLAY_OBS_PITCH), ring_meta(capacity * GBL_REPLAY_META_PITCH);
        std::vector<int16_t> ring_visits(capacity * GBL_REPLAY_VISITS_PITCH);
        std::vector<int32_t> ring_prio(capacity, 0);
        std::vector<uint64_t> index(index_bytes / 8);
        uint64_t state[2] = {0, 0};
        for (int g = 0; g < 3; ++g) {
            int rc = gbl_cpu_replay_append(obs.data(), mask.data(), visits.data(), z.data(), done.data(), mover.data(), n, plies, stride, 64, g,
                                           ring_obs.data(), ring_visits.data(), ring_meta.data(), capacity, state, ws.data(), need, nullptr);
            if (rc) { printf("append: %s\n", gbl_cpu_last_error()); return 1; }
            rc = gbl_cpu_replay_prio_append(visits.data(), z.data(), done.data(), g ? prio_traj.data() : nullptr, 5, n, plies, stride, 64,
                                            ring_prio.data(), capacity, state, ws.data(), need, nullptr);
            if (rc) { printf("prio_append: %s\n", gbl_cpu_last_error()); return 1; }
            rc = gbl_cpu_replay_prio_index(ring_prio.data(), capacity, state, index.data(), index_bytes, nullptr);
            if (rc) { printf("prio_index: %s\n", gbl_cpu_last_error()); return 1; }
            for (int64_t recent : {0, 5, 36}) {
                const int64_t batch = 200;
                std::vector<int8_t> o(batch * 117), m(batch * 54), zz(batch);
                std::vector<int16_t> v(batch * 54), sym(batch);
                std::vector<int32_t> drawn(2 * batch), prio(batch);
                uint64_t total[2];
                rc = gbl_cpu_replay_batch_prio(ring_obs.data(), ring_visits.data(), ring_meta.data(), capacity, state, ring_prio.data(), index.data(),
                                               prio.data(), total, recent, batch, 511, 3, 1, 2, o.data(), m.data(), v.data(), zz.data(),
                                               drawn.data(), sym.data(), nullptr);
                if (rc) { printf("batch_prio: %s\n", gbl_cpu_last_error()); return 1; }
                for (int64_t j = 0; j < batch; ++j) sum += (uint64_t)(uint32_t)drawn[2 * j] + (uint64_t)(uint16_t)v[j * 54] + (uint64_t)prio[j];
                sum += total[0] + total[1];
                if (recent == 36) {  // the drawn rows get new priorities (duplicates among them), one entry names no slot; the index is rebuilt above
                    drawn[0] = -1;
                    drawn[2] = (int32_t)capacity;
                    for (auto &p : prio) p = (int32_t)(lcg(s) >> 22) - 100;
                    rc = gbl_cpu_replay_prio_update(drawn.data(), prio.data(), batch, ring_prio.data(), capacity, nullptr);
                    if (rc) { printf("prio_update: %s\n", gbl_cpu_last_error()); return 1; }
                }
            }
        }
        for (int32_t p : ring_prio) sum += (uint64_t)(uint32_t)p;
        sum += state[0] + index[1];
    }
    printf("replay prio sanitize run: checksum %llu\n", (unsigned long long)sum);
    return 0;
}
