// gbl_cpu_collect_search_cap under AddressSanitizer + UBSan, as a stand-alone program (no Python, no preload):
//   g++ -O1 -g -std=c++17 -mpopcnt -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -Wno-unknown-pragmas \
//       -Wno-attributes -pthread -o selfplay_cap_main scripts/sanitize_selfplay_cap_main.cpp gobblet-rl_amd/csrc/gobblet_cpu.cpp && ./selfplay_cap_main
// 65 boards -- fresh ones and positions 12 masked-random plies in --; then n = 0 / 1 / 65 boards x 5 plies through both layouts,
// evaluator against evaluator and evaluator against random, guard depths (0, 0) and (2, 3), shares (128, 64), (0, 256) and (256, 0)
// with fast budgets (2, 1) under budgets (6, 4) -- the tree of a full ply is larger than the next fast ply's --, a noise weight, the
// sampled plies, every trajectory array NULL in turn.  Every array is a heap block of EXACTLY the elements its cells reach, so a byte
// read or written beyond them is reported.  A run with an array dropped must leave the boards as they were, a fast ply's visits row
// must be zeros, and a window must hold both kinds of ply.  Prints a checksum; any report of a sanitizer fails the run.
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

// `cells` cells of `row` elements in a block that ends with the last cell's last element
template <typename T>
struct Cells {
    std::unique_ptr<char[]> block;
    T *p;
    size_t bytes;
    Cells(int64_t cells, int64_t row, bool given) : p(nullptr), bytes((size_t)cells * row * sizeof(T))
    {
        if (!given) return;
        block.reset(new char[bytes]);
        memset(block.get(), 0x5A, bytes);
        p = reinterpret_cast<T *>(block.get());
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
    const int64_t N = 65;
    std::vector<int8_t> state0(N * GBL_CELLS, 0), to_move0(N, 0), done0(N, 0);
    std::vector<int32_t> turn0(N, 0);
    // boards 13 .. 64: 12 masked-random plies in (no trajectory array is given)
    CHECK(gbl_cpu_collect_search_eval(state0.data() + 13 * GBL_CELLS, to_move0.data() + 13, done0.data() + 13, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N - 13, 64, 64, 3,
                                      13, 0, nullptr, 12, GBL_POLICY_RANDOM, GBL_POLICY_RANDOM, nullptr, nullptr, 0, 0, 16, 0, GBL_ILLEGAL_NOOP,
                                      nullptr, turn0.data() + 13, nullptr));
    for (int64_t b = 13; b < N; ++b) turn0[b] %= 4;
    // two seeded integer networks (H = 64 and 128)
    uint32_t x = 12345;
    auto next = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    std::vector<int8_t> w1[2], w2[2];
    std::vector<int32_t> b1[2], b2[2];
    gbl_evaluator ev[2];
    for (int m = 0; m < 2; ++m) {
        const int hidden = 64 << m;
        w1[m].resize(117 * hidden); w2[m].resize((hidden / 4) * 56 * 4); b1[m].resize(hidden); b2[m].resize(56);
        for (auto &v : w1[m]) v = (int8_t)(next() & 0xFF);
        for (auto &v : w2[m]) v = (int8_t)(next() & 0xFF);
        for (auto &v : b1[m]) v = (int32_t)(next() % 600) - 300;
        for (auto &v : b2[m]) v = (int32_t)(next() % 131072) - 65536;
        ev[m] = gbl_evaluator{w1[m].data(), b1[m].data(), w2[m].data(), b2[m].data(), hidden, 1, 9, 9};
    }

    const int T = 5;
    const int pol[2][2] = {{GBL_POLICY_EVAL_TREE, GBL_POLICY_EVAL_TREE}, {GBL_POLICY_EVAL_TREE, GBL_POLICY_RANDOM}};
    const int deps[2][2] = {{0, 0}, {2, 3}};
    const int shares[3][2] = {{128, 64}, {0, 256}, {256, 0}};
    uint64_t sum = 0;
    const int64_t ns[3] = {0, 1, 65};
    for (int tile = 0; tile < 2; ++tile)
        for (int64_t n : ns)
            for (int which = 0; which < 2; ++which)
                for (int guard = 0; guard < 2; ++guard)
                    for (int sh = 0; sh < 3; ++sh) {
                        uint64_t first = 0;
                        for (int drop = -1; drop < 16; ++drop) {  // which trajectory array is NULL (-1: none)
                            const int64_t tiles = (n + 63) / 64;
                            const int64_t ply_stride = tile ? 64 : tiles * 64 + 16, tile_stride = tile ? 64 * T : 64;
                            // the last cell any board reaches, + 1
                            const int64_t cells = n ? (T - 1) * ply_stride + ((n - 1) >> 6) * tile_stride + ((n - 1) & 63) + 1 : 0;
                            int k = 0;
                            auto given = [&]() { return k++ != drop; };
                            Cells<int32_t> actions(cells, 1, given());
                            Cells<int8_t> winner(cells, 1, given()), reward(cells, 2, given()), done_t(cells, 1, given()),
                                to_move_t(cells, 1, given()), mask(cells, GBL_ACTIONS, given()), obs(cells, GBL_OBS_BYTES, given());
                            Cells<int16_t> visits(cells, GBL_ACTIONS, given());
                            Cells<int32_t> value(cells, 1, given()), nodes(cells, 1, given());
                            Cells<int8_t> how(cells, 1, given()), mover(cells, 1, given());
                            Cells<int32_t> root_value(cells, 1, given());
                            Cells<uint8_t> priors(cells, GBL_ACTIONS, given());
                            Cells<int8_t> outcome(cells, GBL_ACTIONS, given()), proven(cells, 1, given());
                            Cells<int8_t> state(n, GBL_CELLS, true), to_move(n, 1, true), done(n, 1, true);
                            Cells<int32_t> turn(n, 1, true);
                            if (n) {
                                memcpy(state.p, state0.data(), n * GBL_CELLS);
                                memcpy(to_move.p, to_move0.data(), n);
                                memcpy(turn.p, turn0.data(), n * sizeof(int32_t));
                            }
                            CHECK(gbl_cpu_collect_search_cap(state.p, to_move.p, done.p, actions.p, winner.p, reward.p, done_t.p, to_move_t.p, mask.p,
                                                             obs.p, visits.p, value.p, nodes.p, how.p, mover.p, root_value.p, priors.p, outcome.p,
                                                             proven.p, n, ply_stride, tile_stride, 7, 1000, 3, nullptr, T, pol[which][0],
                                                             pol[which][1], &ev[0], which ? nullptr : &ev[1], 6, 4, deps[guard][0], deps[guard][1],
                                                             64, 0, 24, 2, tile ? GBL_ILLEGAL_TERMINATE : GBL_ILLEGAL_NOOP, nullptr, turn.p, 2, 1,
                                                             shares[sh][0], shares[sh][1], nullptr));
                            // what a run leaves on the boards does not depend on which array was given
                            const uint64_t boards = state.sum() * 7 + to_move.sum() * 5 + done.sum() * 3 + turn.sum();
                            if (drop < 0) first = boards;
                            else if (boards != first) {
                                printf("tile %d n %lld policies %d guard %d shares %d: dropping array %d changed the boards\n", tile, (long long)n,
                                       which, guard, sh, drop);
                                return 1;
                            }
                            if (drop >= 0) continue;
                            int fast = 0, full = 0;
                            for (int t = 0; t < T && n; ++t)
                                for (int64_t b = 0; b < n; ++b) {
                                    const int64_t at = t * ply_stride + (b >> 6) * tile_stride + (b & 63);
                                    const int h = how.p[at];
                                    int total = 0;
                                    for (int a = 0; a < GBL_ACTIONS; ++a) total += visits.p[at * GBL_ACTIONS + a];
                                    const bool is_fast = h == GBL_HOW_FAST || h == GBL_HOW_FAST_SAMPLED;
                                    fast += is_fast;
                                    full += h == GBL_HOW_SEARCH || h == GBL_HOW_SEARCH_SAMPLED;
                                    if (is_fast ? total != 0 : (h != GBL_HOW_RANDOM) != (total > 0)) {
                                        printf("cell (%d, %lld): how %d with a visits sum of %d\n", t, (long long)b, h, total);
                                        return 1;
                                    }
                                }
                            // (against a random side the one evaluator side is all fast at share 0 and all full at share 256)
                            if (n == 65 && !((fast || (which && sh == 2)) && (full || (which && sh == 1)))) {
                                printf("tile %d policies %d guard %d shares %d: %d fast and %d full plies\n", tile, which, guard, sh, fast, full);
                                return 1;
                            }
                            sum = sum * 31 + boards + actions.sum() + visits.sum() + how.sum() + nodes.sum() + priors.sum();
                        }
                    }
    printf("selfplay_cap sanitizer run OK, checksum %016llx\n", (unsigned long long)sum);
    return 0;
}
