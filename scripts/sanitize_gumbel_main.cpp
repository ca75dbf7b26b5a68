// gbl_cpu_tree_search_gumbel and gbl_cpu_collect_search_gumbel under AddressSanitizer + UBSan, as a stand-alone program (no Python, no
// preload):
//   g++ -O1 -g -std=c++17 -mpopcnt -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -Wno-unknown-pragmas \
//       -Wno-attributes -pthread -o gumbel_main scripts/sanitize_gumbel_main.cpp gobblet-rl_amd/csrc/gobblet_cpu.cpp && ./gumbel_main
// 65 boards -- fresh ones and positions 12 masked-random plies in.  The single decision: n = 0 / 1 / 65 boards, with and without a mask
// (rows of 54, 2, 1 and 0 candidates among them), (considered, iterations) = (1, 8), (3, 8), (16, 16), (54, 12) and (16, 64), noise off
// and on, (visit_offset, scale) = (50, 23), (255, 64) and (0, 0), every output NULL in turn.  Self-play: n = 0 / 1 / 65 boards x 5 plies
// through both layouts, evaluator against evaluator and against random, considered (16, 0), (0, 4), (3, 54) and (0, 0) under budgets
// (6, 12), every trajectory array NULL in turn.  Every array is a heap block of EXACTLY the elements its rows or cells reach, so a byte
// read or written beyond them is reported.  A run with an array dropped must leave the boards as they were, a Gumbel ply's row must be
// target bytes (1 .. 255 on the candidates, summing to 255 at least) and the decision must lie in the mask.  Prints a checksum; any
// report of a sanitizer fails the run.
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
    uint64_t sum = 0;
    const int64_t ns[3] = {0, 1, 65};

    // ---- the single decision -----------------------------------------------------------------------------------------------------------
    const int pairs[5][2] = {{1, 8}, {3, 8}, {16, 16}, {54, 12}, {16, 64}};
    const int knobs[3][2] = {{50, 23}, {255, 64}, {0, 0}};
    for (int64_t n : ns)
        for (int masked = 0; masked < 2; ++masked)
            for (int pr = 0; pr < 5; ++pr)
                for (int noise = 0; noise < 2; ++noise)
                    for (int kn = 0; kn < 3; ++kn)
                        for (int drop = -1; drop < (pr == 2 ? 9 : 0); ++drop) {  // which output is NULL (-1: none)
                            int k = 0;
                            auto given = [&]() { return k++ != drop; };
                            Cells<int32_t> visits(n, GBL_ACTIONS, given()), wins(n, GBL_ACTIONS, given()), losses(n, GBL_ACTIONS, given()),
                                action(n, 1, given()), nodes(n, 1, given()), root_value(n, 1, given());
                            Cells<uint8_t> priors(n, GBL_ACTIONS, given()), target(n, GBL_ACTIONS, given());
                            Cells<int16_t> gumbel(n, GBL_ACTIONS, given());
                            Cells<int8_t> state(n, GBL_CELLS, true), to_move(n, 1, true), mask(n, GBL_ACTIONS, masked != 0);
                            if (n) {
                                memcpy(state.p, state0.data(), n * GBL_CELLS);
                                memcpy(to_move.p, to_move0.data(), n);
                            }
                            if (masked)  // row b keeps every action, or the first two, the first one or none (any non-zero byte counts as set)
                                for (int64_t b = 0; b < n; ++b)
                                    for (int a = 0; a < GBL_ACTIONS; ++a) {
                                        const int keep = b % 4 == 0 ? 54 : (b % 4 == 1 ? 2 : (b % 4 == 2 ? 1 : 0));
                                        mask.p[b * GBL_ACTIONS + a] = (int8_t)(a < keep ? 1 + (a & 1) * 6 : 0);
                                    }
                            CHECK(gbl_cpu_tree_search_gumbel(state.p, to_move.p, mask.p, &ev[pr & 1], pairs[pr][1], 24, pairs[pr][0], noise,
                                                             knobs[kn][0], knobs[kn][1], 7, (1ull << 41) + 5, 3, visits.p, wins.p, losses.p,
                                                             action.p, nodes.p, root_value.p, priors.p, target.p, gumbel.p, n, nullptr));
                            if (drop >= 0) continue;
                            for (int64_t b = 0; b < n; ++b) {
                                int total = 0, cand = 0, spent = 0;
                                for (int a = 0; a < GBL_ACTIONS; ++a) {
                                    total += target.p[b * GBL_ACTIONS + a];
                                    cand += target.p[b * GBL_ACTIONS + a] != 0;
                                    spent += visits.p[b * GBL_ACTIONS + a];
                                    if (!noise && gumbel.p[b * GBL_ACTIONS + a]) {
                                        printf("board %lld: a Gumbel value without noise\n", (long long)b);
                                        return 1;
                                    }
                                }
                                const int a = action.p[b];
                                const bool ok = cand == 0 ? (a == -1 && spent == 0 && total == 0)
                                                          : (a >= 0 && a < GBL_ACTIONS && target.p[b * GBL_ACTIONS + a] != 0 &&
                                                             visits.p[b * GBL_ACTIONS + a] > 0 && spent == pairs[pr][1] && total >= 255 &&
                                                             (!masked || mask.p[b * GBL_ACTIONS + a]));
                                if (!ok) {
                                    printf("board %lld: action %d, %d candidates, %d iterations spent, a target sum of %d\n", (long long)b, a, cand,
                                           spent, total);
                                    return 1;
                                }
                            }
                            sum = sum * 31 + visits.sum() + wins.sum() + action.sum() + target.sum() + gumbel.sum() + priors.sum();
                        }

    // ---- self-play -----------------------------------------------------------------------------------------------------------------------
    const int T = 5;
    const int pol[2][2] = {{GBL_POLICY_EVAL_TREE, GBL_POLICY_EVAL_TREE}, {GBL_POLICY_EVAL_TREE, GBL_POLICY_RANDOM}};
    const int considered[4][2] = {{16, 0}, {0, 4}, {3, 54}, {0, 0}};
    for (int tile = 0; tile < 2; ++tile)
        for (int64_t n : ns)
            for (int which = 0; which < 2; ++which)
                for (int cs = 0; cs < 4; ++cs) {
                    uint64_t first = 0;
                    for (int drop = -1; drop < 14; ++drop) {  // which trajectory array is NULL (-1: none)
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
                        Cells<int8_t> state(n, GBL_CELLS, true), to_move(n, 1, true), done(n, 1, true);
                        Cells<int32_t> turn(n, 1, true);
                        if (n) {
                            memcpy(state.p, state0.data(), n * GBL_CELLS);
                            memcpy(to_move.p, to_move0.data(), n);
                            memcpy(turn.p, turn0.data(), n * sizeof(int32_t));
                        }
                        CHECK(gbl_cpu_collect_search_gumbel(state.p, to_move.p, done.p, actions.p, winner.p, reward.p, done_t.p, to_move_t.p, mask.p,
                                                            obs.p, visits.p, value.p, nodes.p, how.p, mover.p, root_value.p, priors.p, n, ply_stride,
                                                            tile_stride, 7, 1000, 3, nullptr, T, pol[which][0], pol[which][1], &ev[0],
                                                            which ? nullptr : &ev[1], 6, 12, 24, 2, tile ? GBL_ILLEGAL_TERMINATE : GBL_ILLEGAL_NOOP,
                                                            nullptr, turn.p, considered[cs][0], considered[cs][1], 1 - tile, 50, 23, nullptr));
                        // what a run leaves on the boards does not depend on which array was given
                        const uint64_t boards = state.sum() * 7 + to_move.sum() * 5 + done.sum() * 3 + turn.sum();
                        if (drop < 0) first = boards;
                        else if (boards != first) {
                            printf("tile %d n %lld policies %d considered %d: dropping array %d changed the boards\n", tile, (long long)n, which, cs,
                                   drop);
                            return 1;
                        }
                        if (drop >= 0) continue;
                        int rule = 0, keys = 0;
                        for (int t = 0; t < T && n; ++t)
                            for (int64_t b = 0; b < n; ++b) {
                                const int64_t at = t * ply_stride + (b >> 6) * tile_stride + (b & 63);
                                const int h = how.p[at], m = mover.p[at];
                                int total = 0, high = 0;
                                for (int a = 0; a < GBL_ACTIONS; ++a) {
                                    total += visits.p[at * GBL_ACTIONS + a];
                                    high = visits.p[at * GBL_ACTIONS + a] > high ? visits.p[at * GBL_ACTIONS + a] : high;
                                }
                                const bool gumbel_side = pol[which][m] == GBL_POLICY_EVAL_TREE && considered[cs][m] > 0;
                                rule += h == GBL_HOW_GUMBEL;
                                keys += h == GBL_HOW_SEARCH || h == GBL_HOW_SEARCH_SAMPLED;
                                if ((h == GBL_HOW_GUMBEL) != gumbel_side || (h == GBL_HOW_GUMBEL && total && (total < 255 || high > 255)) ||
                                    (h == GBL_HOW_RANDOM && total)) {
                                    printf("cell (%d, %lld): how %d, mover %d, a row sum of %d (largest %d)\n", t, (long long)b, h, m, total, high);
                                    return 1;
                                }
                            }
                        bool want_rule = false, want_keys = false;  // a side that follows the rule; a side that searches by the keys
                        for (int m = 0; m < 2; ++m)
                            if (pol[which][m] == GBL_POLICY_EVAL_TREE) (considered[cs][m] > 0 ? want_rule : want_keys) = true;
                        if (n == 65 && (want_rule != (rule > 0) || want_keys != (keys > 0))) {
                            printf("tile %d policies %d considered %d: %d Gumbel plies and %d plies by the keys\n", tile, which, cs, rule, keys);
                            return 1;
                        }
                        sum = sum * 31 + boards + actions.sum() + visits.sum() + how.sum() + nodes.sum() + priors.sum();
                    }
                }
    printf("gumbel sanitizer run OK, checksum %016llx\n", (unsigned long long)sum);
    return 0;
}
