// gbl_cpu_reanalyse under AddressSanitizer + UBSan, as a stand-alone program (no Python, no preload):
//   g++ -O1 -g -std=c++17 -mpopcnt -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -Wno-unknown-pragmas \
//       -Wno-attributes -pthread -o reanalyse_main scripts/sanitize_reanalyse_main.cpp gobblet-rl_amd/csrc/gobblet_cpu.cpp && ./reanalyse_main
// Boards of masked-random play seen by their movers (every fifth row all zeros, every seventh with z = GBL_Z_OPEN, every eleventh with an
// empty mask), a network of pseudo-random weights in heap blocks of exactly its sizes, then n = 0 / 1 / 65 rows through both pitch sets
// -- a batch's and the ring's, z inside the mask's rows as in ring_meta --, in place and into outputs of their own, at 1, 8 and 512
// iterations, every optional pointer NULL in turn.  Every array is a heap block of EXACTLY (n - 1) * pitch + row elements, so a byte
// read or written beyond a row's elements is reported; the batch's byte arrays start at odd addresses.  In-place and separate outputs
// must agree.  Prints a checksum; any report of a sanitizer fails the run.
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

// n rows of `row` elements, `pitch` apart, in a block that ends with the last row's last element; `odd`: the block starts sizeof(T) * odd bytes in
template <typename T>
struct Rows {
    std::unique_ptr<char[]> block;
    T *p;
    int64_t pitch;
    Rows(int64_t n, int64_t row, int64_t pitch_, bool odd, int fill) : pitch(pitch_)
    {
        const size_t bytes = n ? ((size_t)(n - 1) * pitch + row) * sizeof(T) : 0, lead = odd ? sizeof(T) : 0;
        block.reset(new char[bytes + lead]);
        memset(block.get(), fill, bytes + lead);
        p = reinterpret_cast<T *>(block.get() + lead);
    }
    char *at(int64_t r) { return reinterpret_cast<char *>(p) + r * pitch * sizeof(T); }
};

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

int main()
{
    const int64_t N = 65;
    const int H = 64;
    std::vector<int8_t> state(N * GBL_CELLS), to_move(N), done(N), obs(N * GBL_OBS_BYTES), legal(N * GBL_ACTIONS);
    CHECK(gbl_cpu_reset(state.data(), to_move.data(), done.data(), nullptr, N, nullptr));
    std::vector<int32_t> act(N);
    for (uint32_t ply = 0; ply < 5; ++ply) {  // (board b stops after b % 6 plies: nobody holds a line before the fifth)
        const std::vector<int8_t> state_was = state, to_move_was = to_move;
        CHECK(gbl_cpu_legal_mask(state.data(), to_move.data(), legal.data(), N, nullptr));
        CHECK(gbl_cpu_sample(legal.data(), act.data(), N, 7, 0, ply, nullptr));
        CHECK(gbl_cpu_play_turn(state.data(), to_move.data(), act.data(), N, nullptr));
        for (int64_t b = 0; b < N; ++b) {
            to_move[b] ^= 1;
            if ((int64_t)ply >= b % 6) {
                memcpy(state.data() + b * GBL_CELLS, state_was.data() + b * GBL_CELLS, GBL_CELLS);
                to_move[b] = to_move_was[b];
            }
        }
    }
    CHECK(gbl_cpu_observe(state.data(), to_move.data(), -1, obs.data(), N, nullptr));
    CHECK(gbl_cpu_legal_mask(state.data(), to_move.data(), legal.data(), N, nullptr));
    for (int64_t b = 4; b < N; b += 5) memset(obs.data() + b * GBL_OBS_BYTES, 0, GBL_OBS_BYTES);
    for (int64_t b = 10; b < N; b += 11) memset(legal.data() + b * GBL_ACTIONS, 0, GBL_ACTIONS);

    // the network in blocks of exactly its sizes
    uint32_t s = 12345u;
    std::unique_ptr<int8_t[]> w1(new int8_t[117 * H]), w2(new int8_t[H * 56]);
    std::unique_ptr<int32_t[]> b1(new int32_t[H]), b2(new int32_t[56]);
    for (int i = 0; i < 117 * H; ++i) w1[i] = (int8_t)(lcg(s) >> 24);
    for (int i = 0; i < H * 56; ++i) w2[i] = (int8_t)(lcg(s) >> 24);
    for (int i = 0; i < H; ++i) b1[i] = (int32_t)(lcg(s) >> 23) - 256;
    for (int i = 0; i < 56; ++i) b2[i] = (int32_t)(lcg(s) >> 15) - 65536;
    const gbl_evaluator ev{w1.get(), b1.get(), w2.get(), b2.get(), H, 1, 9, 9};

    uint64_t sum = 0;
    const int64_t ns[3] = {0, 1, 65};
    const int its[3] = {1, 8, 512};
    for (int ring = 0; ring < 2; ++ring)
        for (int64_t n : ns)
            for (int iterations : its)
                for (int drop = 0; drop < 11; ++drop) {  // which optional pointer is NULL: none, mask, visits_in, z_in, visits_out, then the six dense outputs
                    const int64_t po = ring ? GBL_REPLAY_OBS_PITCH : GBL_OBS_BYTES, pm = ring ? GBL_REPLAY_META_PITCH : GBL_ACTIONS,
                                  pv = ring ? GBL_REPLAY_VISITS_PITCH : GBL_ACTIONS, pz = ring ? GBL_REPLAY_META_PITCH : 1;
                    const bool odd = !ring;
                    int16_t visits[2][65][GBL_ACTIONS];
                    int32_t drift[2][65];
                    for (int inplace = 0; inplace < 2; ++inplace) {
                        Rows<int8_t> o(n, GBL_OBS_BYTES, po, odd, 0x5A), m(n, ring ? GBL_REPLAY_META_Z + 1 : GBL_ACTIONS, pm, odd, 0x5A), z(n, 1, pz, odd, 0x5A),
                            census(n, 1, 1, odd, 0x5A);
                        Rows<uint8_t> priors(n, GBL_ACTIONS, GBL_ACTIONS, odd, 0x5A);
                        Rows<int16_t> v(n, GBL_ACTIONS, pv, odd, 0x5A), v2(n, GBL_ACTIONS, pv, odd, 0x5A);
                        Rows<int32_t> value(n, 1, 1, odd, 0x5A), action(n, 1, 1, odd, 0x5A), nodes(n, 1, 1, odd, 0x5A), moved(n, 1, 1, odd, 0x5A);
                        int8_t *z_in = ring ? m.p + GBL_REPLAY_META_Z : z.p;  // (the ring keeps z in byte 54 of the mask's row)
                        for (int64_t r = 0; r < n; ++r) {
                            memcpy(o.at(r), obs.data() + r * GBL_OBS_BYTES, GBL_OBS_BYTES);
                            memcpy(m.at(r), legal.data() + r * GBL_ACTIONS, GBL_ACTIONS);
                            z_in[r * pz] = (int8_t)(r % 7 == 6 ? GBL_Z_OPEN : (int)(r % 3) - 1);
                            int16_t old[GBL_ACTIONS];
                            for (int a = 0; a < GBL_ACTIONS; ++a) old[a] = (int16_t)(r % 13 == 12 ? 32767 : (r * 31 + a * 17) % 23 - 4);
                            memcpy(v.at(r), old, sizeof old);
                        }
                        const int16_t *vin = drop == 2 ? nullptr : v.p;
                        const int8_t *zin = drop == 3 ? nullptr : z_in;
                        int16_t *vout = drop == 4 ? nullptr : (inplace && vin ? v.p : v2.p);
                        CHECK(gbl_cpu_reanalyse(&ev, iterations, 16, o.p, po, drop == 1 ? nullptr : m.p, pm, vin, vout, pv, zin, pz,
                                                drop == 5 ? nullptr : value.p, drop == 6 ? nullptr : priors.p, drop == 7 ? nullptr : action.p,
                                                drop == 8 ? nullptr : nodes.p, drop == 9 ? nullptr : moved.p, drop == 10 ? nullptr : census.p, n,
                                                nullptr));
                        for (int64_t r = 0; r < n; ++r) {
                            const bool skipped = zin && r % 7 == 6;  // (its visits stay what they were: not comparable)
                            memset(visits[inplace][r], 0, sizeof visits[inplace][r]);
                            if (vout && !skipped) memcpy(visits[inplace][r], reinterpret_cast<char *>(vout) + r * pv * 2, sizeof visits[inplace][r]);
                            drift[inplace][r] = drop == 9 ? 0 : moved.p[r];
                            sum += (uint64_t)(uint16_t)visits[inplace][r][r % GBL_ACTIONS] + (uint64_t)(uint32_t)drift[inplace][r];
                            if (drop != 5) sum += (uint64_t)(uint32_t)value.p[r];
                            if (drop != 6) sum += (uint64_t)priors.p[r * GBL_ACTIONS + r % GBL_ACTIONS];
                            if (drop != 7) sum += (uint64_t)(uint32_t)action.p[r];
                            if (drop != 8) sum += (uint64_t)(uint32_t)nodes.p[r];
                            if (drop != 10) sum += (uint64_t)(uint8_t)census.p[r];
                        }
                    }
                    for (int64_t r = 0; r < n; ++r)
                        if (drift[0][r] != drift[1][r] || memcmp(visits[0][r], visits[1][r], sizeof visits[0][r]) != 0) {
                            printf("in place and separate outputs differ: ring %d n %lld iterations %d drop %d row %lld\n", ring, (long long)n,
                                   iterations, drop, (long long)r);
                            return 1;
                        }
                }
    printf("reanalyse sanitize run: checksum %llu\n", (unsigned long long)sum);
    return 0;
}
