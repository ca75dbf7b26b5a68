// The host flavour's tablebase entry points under AddressSanitizer + UBSan, as a stand-alone program (scripts/sanitize_cpu.sh builds it
// together with csrc/gobblet_cpu.cpp and runs it): prepare into an exactly-sized heap block, the (1, 1, 1) universe (753 571 positions)
// built in place in ragged slices -- 1, 63 and 65 positions, the middle, a last slice that ends at the last position -- and, beside it,
// (2, 0, 1) sweep by sweep into a buffer of its own; the round trip index -> position -> index over a whole universe, and a probe with
// and without a mask and with NULL outputs.  Prints a checksum; any report of a sanitizer fails the run.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../include/gobblet_cpu.h"

#define CHECK(call)                                                 \
    do {                                                            \
        if ((call) != 0) {                                          \
            printf("%s: %s\n", #call, gbl_cpu_last_error());        \
            return 1;                                               \
        }                                                           \
    } while (0)

int main()
{
    uint64_t sum = 0;
    std::vector<uint8_t> aux(GBL_TB_AUX_BYTES);
    {
        const int32_t inv[3] = {1, 1, 1};
        const int64_t positions = 91 * 91 * 91;
        CHECK(gbl_cpu_tb_prepare(inv, aux.data(), nullptr));
        std::vector<int8_t> table(positions);
        const int64_t cuts[] = {0, 1, 64, 129, positions - 1000, positions};
        for (int k = 0; k <= GBL_TB_MAX_SWEEP; ++k) {
            uint64_t decided = 0;
            for (int i = 0; i + 1 < 6; ++i)
                CHECK(gbl_cpu_tb_sweep(inv, aux.data(), k <= 1 ? nullptr : table.data(), table.data() + cuts[i], cuts[i], cuts[i + 1] - cuts[i], k,
                                       &decided, nullptr));
            sum += decided * (uint64_t)(k + 1);
            if (k > 0 && decided == 0) break;
        }
        const int64_t n = 4097;
        std::vector<int64_t> index(n), back(n);
        for (int64_t b = 0; b < n; ++b) index[b] = (b * 184) % positions;
        index[0] = positions - 1;
        index[1] = positions;  // outside: a row of GBL_TB_TERMINAL, whose index is -1
        std::vector<int8_t> state(n * GBL_CELLS), to_move(n, 0), mask(n * GBL_ACTIONS), outcome(n * GBL_ACTIONS), value(n);
        std::vector<int32_t> action(n);
        CHECK(gbl_cpu_tb_position(inv, aux.data(), index.data(), state.data(), n, nullptr));
        for (int64_t b = 1; b < n; b += 2) {  // every other board from player_2's side
            to_move[b] = 1;
            for (int c = 0; c < GBL_CELLS; ++c) state[b * GBL_CELLS + c] = (int8_t)-state[b * GBL_CELLS + c];
        }
        CHECK(gbl_cpu_tb_index(inv, aux.data(), state.data(), to_move.data(), back.data(), n, nullptr));
        for (int64_t b = 0; b < n; ++b)
            if (back[b] != (b == 1 ? -1 : index[b])) {
                printf("round trip failed at %lld\n", (long long)b);
                return 1;
            }
        for (size_t i = 0; i < mask.size(); ++i) mask[i] = (int8_t)(i % 3 != 0);
        CHECK(gbl_cpu_tb_probe(inv, aux.data(), table.data(), state.data(), to_move.data(), nullptr, outcome.data(), value.data(), action.data(), n,
                               nullptr));
        for (int64_t b = 0; b < n; ++b) sum += (uint64_t)(uint8_t)value[b] + (uint64_t)(uint32_t)action[b] + (uint64_t)(uint8_t)outcome[b * GBL_ACTIONS + 7];
        CHECK(gbl_cpu_tb_probe(inv, aux.data(), table.data(), state.data(), to_move.data(), mask.data(), nullptr, value.data(), nullptr, n, nullptr));
        for (int64_t b = 0; b < n; ++b) sum += (uint64_t)(uint8_t)value[b];
    }
    {
        const int32_t inv[3] = {2, 0, 1};
        const int64_t positions = 1423 * 91;
        std::vector<int8_t> table(positions), next(positions);
        for (int k = 0; k < 4; ++k) {
            uint64_t decided = 0;
            next = table;
            CHECK(gbl_cpu_tb_sweep(inv, aux.data(), table.data(), next.data(), 0, positions, k, &decided, nullptr));
            table = next;
            sum += decided;
        }
    }
    printf("tablebase sanitize run: checksum %llu\n", (unsigned long long)sum);
    return 0;
}
