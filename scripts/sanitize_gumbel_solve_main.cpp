// gbl_cpu_collect_gumbel_solve under AddressSanitizer + UBSan, as a stand-alone program (no Python, no preload; it runs on the CPU only):
//   g++ -O1 -g -std=c++17 -mpopcnt -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -Wno-unknown-pragmas \
//       -Wno-attributes -pthread -o gumbel_solve_main scripts/sanitize_gumbel_solve_main.cpp gobblet-rl_amd/csrc/gobblet_cpu.cpp && ./gumbel_solve_main
// 65 boards -- fresh ones and positions 40 masked-random plies in, where the solver proves wins and losses.  n = 0 / 1 / 65 boards x 5
// plies through both layouts, evaluator against evaluator and against random, (considered, depths) = ((16, 16), (2, 3)), ((16, 0), (3, 3)),
// ((3, 54), (0, 2)), ((4, 4), (3, 0)), ((0, 0), (2, 2)) and ((16, 4), (0, 0)) under budgets (6, 12), every one of the 16 trajectory arrays
// NULL in turn.  Every array is a heap block of EXACTLY the elements its cells reach, so a byte read or written beyond them is reported.
// A run with an array dropped must leave the boards as they were; a proven ply must carry a one-hot row at the budget and a non-zero V,
// a Gumbel ply of a guarded side target bytes exactly on the actions of outcome 0 and an action among them, and an unguarded ply an
// outcome row of GBL_SOLVE_NONE.  Prints a checksum; any report of a sanitizer fails the run.
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
    // boards 5 .. 64: 40 masked-random plies in (no trajectory array is given)
    CHECK(gbl_cpu_collect_search_eval(state0.data() + 5 * GBL_CELLS, to_move0.data() + 5, done0.data() + 5, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N - 5, 64, 64, 3,
                                      5, 0, nullptr, 40, GBL_POLICY_RANDOM, GBL_POLICY_RANDOM, nullptr, nullptr, 0, 0, 16, 0, GBL_ILLEGAL_NOOP,
                                      nullptr, turn0.data() + 5, nullptr));
    for (int64_t b = 5; b < N; ++b) turn0[b] %= 4;
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
    const int T = 5, budget[2] = {6, 12};
    const int pol[2][2] = {{GBL_POLICY_EVAL_TREE, GBL_POLICY_EVAL_TREE}, {GBL_POLICY_EVAL_TREE, GBL_POLICY_RANDOM}};
    const int considered[6][2] = {{16, 16}, {16, 0}, {3, 54}, {4, 4}, {0, 0}, {16, 4}};
    const int depths[6][2] = {{2, 3}, {3, 3}, {0, 2}, {3, 0}, {2, 2}, {0, 0}};
    int met_proven = 0, met_rule = 0, met_subset = 0, met_keys = 0;
    for (int tile = 0; tile < 2; ++tile)
        for (int64_t n : ns)
            for (int which = 0; which < 2; ++which)
                for (int cs = 0; cs < 6; ++cs) {
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
                        CHECK(gbl_cpu_collect_gumbel_solve(state.p, to_move.p, done.p, actions.p, winner.p, reward.p, done_t.p, to_move_t.p, mask.p,
                                                           obs.p, visits.p, value.p, nodes.p, how.p, mover.p, root_value.p, priors.p, outcome.p,
                                                           proven.p, n, ply_stride, tile_stride, 7, 1000, 3, nullptr, T, pol[which][0], pol[which][1],
                                                           &ev[0], which ? nullptr : &ev[1], budget[0], budget[1], depths[cs][0], depths[cs][1], 24,
                                                           2, tile ? GBL_ILLEGAL_TERMINATE : GBL_ILLEGAL_NOOP, nullptr, turn.p, considered[cs][0],
                                                           considered[cs][1], 1 - tile, 50, 23, nullptr));
                        // what a run leaves on the boards does not depend on which array was given
                        const uint64_t boards = state.sum() * 7 + to_move.sum() * 5 + done.sum() * 3 + turn.sum();
                        if (drop < 0) first = boards;
                        else if (boards != first) {
                            printf("tile %d n %lld policies %d case %d: dropping array %d changed the boards\n", tile, (long long)n, which, cs, drop);
                            return 1;
                        }
                        if (drop >= 0) continue;
                        for (int t = 0; t < T && n; ++t)
                            for (int64_t b = 0; b < n; ++b) {
                                const int64_t at = t * ply_stride + (b >> 6) * tile_stride + (b & 63);
                                const int h = how.p[at], m = mover.p[at], a = actions.p[at], V = proven.p[at];
                                const bool searches = pol[which][m] == GBL_POLICY_EVAL_TREE, guarded = searches && depths[cs][m] > 0;
                                int total = 0, off = 0, open = 0, none = 0, legal = 0;  // (off: a non-zero byte off the actions of outcome 0)
                                for (int c = 0; c < GBL_ACTIONS; ++c) {
                                    const int v = visits.p[at * GBL_ACTIONS + c], o = outcome.p[at * GBL_ACTIONS + c];
                                    total += v;
                                    open += o == 0;
                                    none += o == GBL_SOLVE_NONE;
                                    off += v != 0 && o != 0;
                                    legal += v != 0;
                                }
                                bool ok;
                                if (!guarded || none == GBL_ACTIONS)  // no guard (or a root without a candidate): an empty outcome row, V = 0
                                    ok = none == GBL_ACTIONS && V == 0 && h != GBL_HOW_PROVEN && (searches || (h == GBL_HOW_RANDOM && total == 0));
                                else if (V != 0)
                                    ok = h == GBL_HOW_PROVEN && a >= 0 && a < GBL_ACTIONS && visits.p[at * GBL_ACTIONS + a] == budget[m] &&
                                         total == budget[m] && legal == 1 && nodes.p[at] == 0 && root_value.p[at] == 0 &&
                                         value.p[at] == (V > 0 ? 128 : -128) * budget[m];
                                else if (considered[cs][m] > 0)
                                    ok = h == GBL_HOW_GUMBEL && open > 0 && off == 0 && legal == open && total >= 255 && a >= 0 &&
                                         outcome.p[at * GBL_ACTIONS + a] == 0;
                                else
                                    ok = (h == GBL_HOW_SEARCH || h == GBL_HOW_SEARCH_SAMPLED) && open > 0 && off == 0 && total == budget[m] &&
                                         a >= 0 && outcome.p[at * GBL_ACTIONS + a] == 0;
                                if (!ok) {
                                    printf("tile %d policies %d case %d cell (%d, %lld): how %d, mover %d, action %d, V %d, a row sum of %d, %d actions "
                                           "of outcome 0, %d bytes off them\n", tile, which, cs, t, (long long)b, h, m, a, V, total, open, off);
                                    return 1;
                                }
                                met_proven += h == GBL_HOW_PROVEN;
                                met_rule += guarded && h == GBL_HOW_GUMBEL;
                                met_subset += guarded && h == GBL_HOW_GUMBEL && open + none < GBL_ACTIONS;
                                met_keys += guarded && (h == GBL_HOW_SEARCH || h == GBL_HOW_SEARCH_SAMPLED);
                            }
                        sum = sum * 31 + boards + actions.sum() + visits.sum() + how.sum() + nodes.sum() + priors.sum() + outcome.sum() + proven.sum();
                    }
                }
    if (!met_proven || !met_rule || !met_subset || !met_keys) {
        printf("a branch was not met: %d proven plies, %d guarded Gumbel plies (%d over a strict subset), %d guarded plies by the keys\n", met_proven,
               met_rule, met_subset, met_keys);
        return 1;
    }
    printf("gumbel-solve sanitizer run OK (%d proven, %d guarded Gumbel, %d over a strict subset, %d by the keys), checksum %016llx\n", met_proven,
           met_rule, met_subset, met_keys, (unsigned long long)sum);
    return 0;
}
