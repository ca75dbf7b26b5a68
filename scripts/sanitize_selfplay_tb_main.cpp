// gbl_cpu_collect_search_tb under AddressSanitizer + UBSan, as a stand-alone program (no Python, no preload):
//   g++ -O1 -g -std=c++17 -mpopcnt -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -Wno-unknown-pragmas \
//       -Wno-attributes -pthread -o selfplay_tb_main scripts/sanitize_selfplay_tb_main.cpp gobblet-rl_amd/csrc/gobblet_cpu.cpp && ./selfplay_tb_main
// The (2, 1, 0) universe built in place; 65 boards -- positions of the universe seen by both movers, boards with a piece the
// inventory lacks (the a* == -1 path) and fresh boards --; then n = 0 / 1 / 65 boards x 5 plies through both layouts, table against
// table, table against random and an evaluator side (guard depth 2, a noise weight) against the table, both modes, the sampled plies,
// every trajectory array NULL in turn.  Every array is a heap block of EXACTLY the elements its cells reach, so a byte read or written
// beyond them is reported; the judge arrays start at odd addresses.  A run with an array dropped must leave the others as they were.
// Prints a checksum; any report of a sanitizer fails the run.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../include/gobblet_cpu.h"

#define CHECK(call)                                                 \
    do {                                                            \
        if ((call) != 0) {                                          \
            printf("%s: %s\n", #call, gbl_cpu_last_error());        \
            return 1;                                               \
        }                                                           \
    } while (0)

// `cells` cells of `row` elements in a block that ends with the last cell's last element; `odd`: the block starts one byte in
template <typename T>
struct Cells {
    std::unique_ptr<char[]> block;
    T *p;
    size_t bytes;
    Cells(int64_t cells, int64_t row, bool odd, bool given) : p(nullptr), bytes((size_t)cells * row * sizeof(T))
    {
        if (!given) return;
        block.reset(new char[bytes + odd]);
        memset(block.get(), 0x5A, bytes + odd);
        p = reinterpret_cast<T *>(block.get() + odd);
    }
    uint64_t sum() const
    {
        uint64_t s = 0;
        if (p)
            for (size_t i = 0; i < bytes; ++i) s = s * 131 + reinterpret_cast<const uint8_t *>(p)[i];
        return s;
    }
};

int main()
{
    const int32_t inv[3] = {2, 1, 0};
    const int64_t positions = 1423 * 91;
    std::vector<uint8_t> aux(GBL_TB_AUX_BYTES);
    CHECK(gbl_cpu_tb_prepare(inv, aux.data(), nullptr));
    std::vector<int8_t> table(positions);
    for (int k = 0; k <= GBL_TB_MAX_SWEEP; ++k) {
        uint64_t decided = 0;
        CHECK(gbl_cpu_tb_sweep(inv, aux.data(), table.data(), table.data(), 0, positions, k, &decided, nullptr));
        if (k > 0 && decided == 0) break;
    }
    const int64_t N = 65;
    std::vector<int64_t> index(N);
    for (int64_t b = 0; b < N; ++b) index[b] = (b * 1987 + 11) % positions;
    std::vector<int8_t> state0(N * GBL_CELLS), to_move0(N);
    std::vector<int32_t> turn0(N);
    CHECK(gbl_cpu_tb_position(inv, aux.data(), index.data(), state0.data(), N, nullptr));
    for (int64_t b = 0; b < N; ++b) {
        to_move0[b] = (int8_t)(b & 1);
        turn0[b] = (int32_t)(b % 4);
        int8_t *s = state0.data() + b * GBL_CELLS;
        for (int c = 0; c < GBL_CELLS; ++c) s[c] = (int8_t)(b % 5 == 4 ? 0 : (b & 1 ? -s[c] : s[c]));  // every fifth board fresh
        if (b % 5 == 4) { to_move0[b] = 0; turn0[b] = 0; }
        if (b % 7 == 3 && s[26] == 0 && s[17] == 0 && s[8] == 0) s[26] = 5;  // a large piece: no state of (2, 1, 0)
    }
    // one seeded integer network (H = 64)
    std::vector<int8_t> w1(117 * 64), w2(16 * 56 * 4);
    std::vector<int32_t> b1(64), b2(56);
    uint32_t x = 12345;
    auto next = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (auto &v : w1) v = (int8_t)(next() & 0xFF);
    for (auto &v : w2) v = (int8_t)(next() & 0xFF);
    for (auto &v : b1) v = (int32_t)(next() % 600) - 300;
    for (auto &v : b2) v = (int32_t)(next() % 131072) - 65536;
    gbl_evaluator ev{w1.data(), b1.data(), w2.data(), b2.data(), 64, 1, 9, 9};

    const int T = 5;
    const int pol[3][2] = {{GBL_POLICY_TABLEBASE, GBL_POLICY_TABLEBASE}, {GBL_POLICY_TABLEBASE, GBL_POLICY_RANDOM},
                           {GBL_POLICY_EVAL_TREE, GBL_POLICY_TABLEBASE}};
    uint64_t sum = 0;
    const int64_t ns[3] = {0, 1, 65};
    for (int tile = 0; tile < 2; ++tile)
        for (int64_t n : ns)
            for (int which = 0; which < 3; ++which)
                for (int mode = 0; mode < 2; ++mode) {
                    uint64_t first = 0;
                    for (int drop = -1; drop < 19; ++drop) {  // which trajectory array is NULL (-1: none)
                        const int64_t tiles = (n + 63) / 64;
                        const int64_t ply_stride = tile ? 64 : tiles * 64 + 16, tile_stride = tile ? 64 * T : 64;
                        // the last cell any board reaches, + 1
                        const int64_t cells = n ? (T - 1) * ply_stride + ((n - 1) >> 6) * tile_stride + ((n - 1) & 63) + 1 : 0;
                        int k = 0;
                        auto given = [&]() { return k++ != drop; };
                        Cells<int32_t> actions(cells, 1, false, given());
                        Cells<int8_t> winner(cells, 1, false, given()), reward(cells, 2, false, given()), done_t(cells, 1, false, given()),
                            to_move_t(cells, 1, false, given()), mask(cells, GBL_ACTIONS, false, given()), obs(cells, GBL_OBS_BYTES, false, given());
                        Cells<int16_t> visits(cells, GBL_ACTIONS, false, given());
                        Cells<int32_t> value(cells, 1, false, given()), nodes(cells, 1, false, given());
                        Cells<int8_t> how(cells, 1, false, given()), mover(cells, 1, false, given());
                        Cells<int32_t> root_value(cells, 1, false, given());
                        Cells<uint8_t> priors(cells, GBL_ACTIONS, false, given());
                        Cells<int8_t> outcome(cells, GBL_ACTIONS, false, given()), proven(cells, 1, false, given());
                        Cells<int8_t> tb_outcome(cells, GBL_ACTIONS, true, given()), tb_value(cells, 1, true, given()), tb_played(cells, 1, true, given());
                        Cells<int8_t> state(n, GBL_CELLS, false, true), to_move(n, 1, false, true), done(n, 1, false, true);
                        Cells<int32_t> turn(n, 1, false, true);
                        if (n) {
                            memcpy(state.p, state0.data(), n * GBL_CELLS);
                            memcpy(to_move.p, to_move0.data(), n);
                            memcpy(turn.p, turn0.data(), n * sizeof(int32_t));
                        }
                        CHECK(gbl_cpu_collect_search_tb(state.p, to_move.p, done.p, actions.p, winner.p, reward.p, done_t.p, to_move_t.p, mask.p,
                                                        obs.p, visits.p, value.p, nodes.p, how.p, mover.p, root_value.p, priors.p, outcome.p,
                                                        proven.p, n, ply_stride, tile_stride, 7, 1000, 3, nullptr, T, pol[which][0], pol[which][1],
                                                        &ev, nullptr, 6, 0, 2, 0, 64, 0, 24, 2, mode ? GBL_ILLEGAL_TERMINATE : GBL_ILLEGAL_NOOP,
                                                        nullptr, turn.p, inv, aux.data(), table.data(), mode, mode ? 600 : 1, tb_outcome.p,
                                                        tb_value.p, tb_played.p, nullptr));
                        // what a run leaves on the boards does not depend on which array was given
                        const uint64_t boards = state.sum() * 7 + to_move.sum() * 5 + done.sum() * 3 + turn.sum();
                        if (drop < 0) first = boards;
                        else if (boards != first) {
                            printf("tile %d n %lld policies %d mode %d: dropping array %d changed the boards\n", tile, (long long)n, which, mode, drop);
                            return 1;
                        }
                        if (drop < 0)
                            sum = sum * 31 + boards + actions.sum() + visits.sum() + how.sum() + tb_outcome.sum() + tb_value.sum() + tb_played.sum();
                    }
                }
    printf("selfplay_tb sanitizer run OK, checksum %016llx\n", (unsigned long long)sum);
    return 0;
}
