// gbl_cpu_collect_gumbel_tb under AddressSanitizer + UBSan, as a stand-alone program (no Python, no preload; it runs on the CPU only):
//   g++ -O1 -g -std=c++17 -mpopcnt -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -Wno-unknown-pragmas \
//       -Wno-attributes -pthread -o gumbel_tb_main scripts/sanitize_gumbel_tb_main.cpp gobblet-rl_amd/csrc/gobblet_cpu.cpp && ./gumbel_tb_main
// The (2, 1, 0) universe built in place; 65 boards -- positions of the universe seen by both movers, boards with a piece the inventory
// lacks (the a* == -1 path) and fresh boards --; then n = 0 / 1 / 65 boards x 5 plies through both layouts on the issue's six cases
// (policies; considered) = (EVAL, TB; 16), (TB, EVAL; 3), (EVAL, EVAL; 16, 0), (EVAL, RANDOM; 54), (TB, TB), (TB, RANDOM) under budgets
// (6, 12), both table modes, the sampled plies, every one of the 17 trajectory arrays NULL in turn.  Every array is a heap block of
// EXACTLY the elements its cells reach, so a byte read or written beyond them is reported; the judge arrays start at odd addresses.  A
// run with an array dropped must leave the boards as they were; tb_played must be the outcome byte of the action played; a table ply
// must carry tb_count on its row, no nodes and no priors, and a Gumbel ply target bytes of 1 .. 255.  Prints a checksum; any report of a
// sanitizer fails the run.
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
    const int E = GBL_POLICY_EVAL_TREE, TB = GBL_POLICY_TABLEBASE, RND = GBL_POLICY_RANDOM;
    const int pol[6][2] = {{E, TB}, {TB, E}, {E, E}, {E, RND}, {TB, TB}, {TB, RND}};
    const int considered[6][2] = {{16, 0}, {0, 3}, {16, 0}, {54, 0}, {0, 0}, {0, 0}};
    const int T = 5, budget[2] = {6, 12};
    uint64_t sum = 0;
    const int64_t ns[3] = {0, 1, 65};
    int met_table = 0, met_sampled = 0, met_rule = 0, met_judged_rule = 0, met_keys = 0, met_random_table = 0, met_none = 0;
    for (int tile = 0; tile < 2; ++tile)
        for (int64_t n : ns)
            for (int cs = 0; cs < 6; ++cs) {
                const int mode = (cs + tile) & 1, count = mode ? 600 : 3;
                uint64_t first = 0;
                for (int drop = -1; drop < 17; ++drop) {  // which trajectory array is NULL (-1: none)
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
                    Cells<int8_t> tb_outcome(cells, GBL_ACTIONS, true, given()), tb_value(cells, 1, true, given()), tb_played(cells, 1, true, given());
                    Cells<int8_t> state(n, GBL_CELLS, false, true), to_move(n, 1, false, true), done(n, 1, false, true);
                    Cells<int32_t> turn(n, 1, false, true);
                    if (n) {
                        memcpy(state.p, state0.data(), n * GBL_CELLS);
                        memcpy(to_move.p, to_move0.data(), n);
                        memcpy(turn.p, turn0.data(), n * sizeof(int32_t));
                    }
                    CHECK(gbl_cpu_collect_gumbel_tb(state.p, to_move.p, done.p, actions.p, winner.p, reward.p, done_t.p, to_move_t.p, mask.p, obs.p,
                                                    visits.p, value.p, nodes.p, how.p, mover.p, root_value.p, priors.p, n, ply_stride, tile_stride, 7,
                                                    1000, 3, nullptr, T, pol[cs][0], pol[cs][1], pol[cs][0] == E ? &ev[0] : nullptr,
                                                    pol[cs][1] == E ? &ev[1] : nullptr, budget[0], budget[1], 24, 2,
                                                    tile ? GBL_ILLEGAL_TERMINATE : GBL_ILLEGAL_NOOP, nullptr, turn.p, considered[cs][0],
                                                    considered[cs][1], 1 - tile, 50, tile ? 0 : 23, inv, aux.data(), table.data(), mode, count,
                                                    tb_outcome.p, tb_value.p, tb_played.p, nullptr));
                    // what a run leaves on the boards does not depend on which array was given
                    const uint64_t boards = state.sum() * 7 + to_move.sum() * 5 + done.sum() * 3 + turn.sum();
                    if (drop < 0) first = boards;
                    else if (boards != first) {
                        printf("tile %d n %lld case %d: dropping array %d changed the boards\n", tile, (long long)n, cs, drop);
                        return 1;
                    }
                    if (drop >= 0) continue;
                    for (int t = 0; t < T && n; ++t)
                        for (int64_t b = 0; b < n; ++b) {
                            const int64_t at = t * ply_stride + (b >> 6) * tile_stride + (b & 63);
                            const int h = how.p[at], m = mover.p[at], a = actions.p[at];
                            int total = 0, on = 0, none = 0, low = 1000, high = 0, pri = 0;
                            for (int c = 0; c < GBL_ACTIONS; ++c) {
                                const int v = visits.p[at * GBL_ACTIONS + c];
                                total += v;
                                on += v != 0;
                                if (v) { low = v < low ? v : low; high = v > high ? v : high; }
                                none += tb_outcome.p[at * GBL_ACTIONS + c] == GBL_SOLVE_NONE;
                                pri += priors.p[at * GBL_ACTIONS + c];
                            }
                            const int played = tb_played.p[at];
                            bool ok = played == (a >= 0 ? tb_outcome.p[at * GBL_ACTIONS + a] : GBL_SOLVE_NONE);  // (every ply is judged here)
                            if (none == GBL_ACTIONS) ok = ok && tb_value.p[at] == 0;
                            if (h == GBL_HOW_TABLE || h == GBL_HOW_TABLE_SAMPLED)
                                ok = ok && pol[cs][m] == TB && on > 0 && low == count && high == count && nodes.p[at] == 0 && root_value.p[at] == 0 &&
                                     pri == 0 && a >= 0 && visits.p[at * GBL_ACTIONS + a] == count && none < GBL_ACTIONS;
                            else if (h == GBL_HOW_GUMBEL)
                                ok = ok && pol[cs][m] == E && considered[cs][m] > 0 && (on == 0 ? a == -1 : (low >= 1 && high <= 255 && total >= 255 && a >= 0));
                            else if (h == GBL_HOW_SEARCH || h == GBL_HOW_SEARCH_SAMPLED)
                                ok = ok && pol[cs][m] == E && considered[cs][m] == 0 && total == (on ? budget[m] : 0);
                            else
                                ok = ok && h == GBL_HOW_RANDOM && pol[cs][m] != E && total == 0 && nodes.p[at] == 0 && pri == 0;
                            if (!ok) {
                                printf("tile %d case %d cell (%d, %lld): how %d, mover %d, action %d, tb_value %d, tb_played %d, a row sum of %d on %d "
                                       "actions\n", tile, cs, t, (long long)b, h, m, a, tb_value.p[at], played, total, on);
                                return 1;
                            }
                            met_table += h == GBL_HOW_TABLE;
                            met_sampled += h == GBL_HOW_TABLE_SAMPLED;
                            met_rule += h == GBL_HOW_GUMBEL;
                            met_judged_rule += h == GBL_HOW_GUMBEL && played != GBL_SOLVE_NONE;
                            met_keys += (h == GBL_HOW_SEARCH || h == GBL_HOW_SEARCH_SAMPLED) && (considered[cs][0] || considered[cs][1]);
                            met_random_table += h == GBL_HOW_RANDOM && pol[cs][m] == TB;
                            met_none += none == GBL_ACTIONS;
                        }
                    sum = sum * 31 + boards + actions.sum() + visits.sum() + how.sum() + nodes.sum() + priors.sum() + tb_outcome.sum() + tb_value.sum() +
                          tb_played.sum();
                }
            }
    if (!met_table || !met_sampled || !met_rule || !met_judged_rule || !met_keys || !met_random_table || !met_none) {
        printf("a branch was not met: %d / %d table plies (plain / sampled), %d Gumbel plies (%d with a verdict of the action), %d plies by the "
               "keys beside the rule, %d random plies of a table side, %d empty verdict rows\n", met_table, met_sampled, met_rule, met_judged_rule,
               met_keys, met_random_table, met_none);
        return 1;
    }
    printf("gumbel-tb sanitizer run OK (%d / %d table plies, %d Gumbel plies, %d of them judged, %d by the keys, %d random plies of a table side, "
           "%d empty verdict rows), checksum %016llx\n", met_table, met_sampled, met_rule, met_judged_rule, met_keys, met_random_table, met_none,
           (unsigned long long)sum);
    return 0;
}
