// gbl_cpu_reanalyse_gumbel under AddressSanitizer + UBSan, as a stand-alone program (no Python, no preload):
//   g++ -O1 -g -std=c++17 -mpopcnt -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -Wno-unknown-pragmas \
//       -Wno-attributes -pthread -o reanalyse_gumbel_main scripts/sanitize_reanalyse_gumbel_main.cpp gobblet-rl_amd/csrc/gobblet_cpu.cpp && ./reanalyse_gumbel_main
// scripts/sanitize_reanalyse_main.cpp's rows -- boards of masked-random play seen by their movers, every fifth row all zeros, every
// seventh with z = GBL_Z_OPEN, every eleventh with an empty mask -- and its network in heap blocks of exactly its sizes, then n = 0 / 1 /
// 65 rows through both pitch sets (a batch's, and the ring's in place with z inside the mask's rows as in ring_meta), at (considered,
// iterations) = (1, 8), (16, 16) and (54, 64), with and without noise, every optional pointer NULL in turn (gumbel_out among them).  Every
// array is a heap block of EXACTLY (n - 1) * pitch + row elements, so a byte read or written beyond a row's elements is reported; the
// batch's byte arrays start at odd addresses.  Every thirteenth row's old visits are 32767 on all 54 actions: the largest So there is,
// 54 * 32767, against the largest Sn the target rule writes (|C| + 254) -- the drift's largest operands an entry point can meet (the sum
// then stays below 2^32: the header's bound beyond it is the bytes' own range; UBSan watches the products either way).  The drift is
// recomputed here in unsigned __int128 from the rows read back.  In-place and separate outputs must agree without noise and with it.
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

// the header's quotient from an old and a new row, in 128 bits
static int32_t drift_of(const int16_t *old, const int16_t *now)
{
    unsigned __int128 So = 0, Sn = 0, diff = 0;
    for (int a = 0; a < GBL_ACTIONS; ++a) {
        So += (unsigned)(old[a] > 0 ? old[a] : 0);
        Sn += (unsigned)now[a];
    }
    if (!Sn) return -1;
    if (!So) return 1024;
    for (int a = 0; a < GBL_ACTIONS; ++a) {
        const unsigned __int128 x = (unsigned __int128)(unsigned)(old[a] > 0 ? old[a] : 0) * Sn, y = (unsigned __int128)(unsigned)now[a] * So;
        diff += x > y ? x - y : y - x;
    }
    return (int32_t)(1024 * diff / (2 * So * Sn));
}

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
    int64_t drifts = 0, largest = 0;
    const int64_t ns[3] = {0, 1, 65};
    const int rule[3][2] = {{1, 8}, {16, 16}, {54, 64}};  // considered, iterations
    for (int ring = 0; ring < 2; ++ring)
        for (int64_t n : ns)
            for (const auto &ci : rule)
                for (int noise = 0; noise < 2; ++noise)
                    for (int drop = 0; drop < 12; ++drop) {  // which optional pointer is NULL: none, mask, visits_in, z_in, visits_out, then the seven dense outputs
                        const int64_t po = ring ? GBL_REPLAY_OBS_PITCH : GBL_OBS_BYTES, pm = ring ? GBL_REPLAY_META_PITCH : GBL_ACTIONS,
                                      pv = ring ? GBL_REPLAY_VISITS_PITCH : GBL_ACTIONS, pz = ring ? GBL_REPLAY_META_PITCH : 1;
                        const bool odd = !ring;
                        int16_t visits[2][65][GBL_ACTIONS];
                        int32_t drift[2][65];
                        for (int inplace = 0; inplace < 2; ++inplace) {
                            Rows<int8_t> o(n, GBL_OBS_BYTES, po, odd, 0x5A), m(n, ring ? GBL_REPLAY_META_Z + 1 : GBL_ACTIONS, pm, odd, 0x5A),
                                z(n, 1, pz, odd, 0x5A), census(n, 1, 1, odd, 0x5A);
                            Rows<uint8_t> priors(n, GBL_ACTIONS, GBL_ACTIONS, odd, 0x5A);
                            Rows<int16_t> v(n, GBL_ACTIONS, pv, odd, 0x5A), v2(n, GBL_ACTIONS, pv, odd, 0x5A), gum(n, GBL_ACTIONS, GBL_ACTIONS, odd, 0x5A);
                            Rows<int32_t> value(n, 1, 1, odd, 0x5A), action(n, 1, 1, odd, 0x5A), nodes(n, 1, 1, odd, 0x5A), moved(n, 1, 1, odd, 0x5A);
                            int8_t *z_in = ring ? m.p + GBL_REPLAY_META_Z : z.p;  // (the ring keeps z in byte 54 of the mask's row)
                            std::vector<int16_t> olds(n * GBL_ACTIONS);
                            for (int64_t r = 0; r < n; ++r) {
                                memcpy(o.at(r), obs.data() + r * GBL_OBS_BYTES, GBL_OBS_BYTES);
                                memcpy(m.at(r), legal.data() + r * GBL_ACTIONS, GBL_ACTIONS);
                                z_in[r * pz] = (int8_t)(r % 7 == 6 ? GBL_Z_OPEN : (int)(r % 3) - 1);
                                int16_t *old = olds.data() + r * GBL_ACTIONS;
                                for (int a = 0; a < GBL_ACTIONS; ++a) old[a] = (int16_t)(r % 13 == 12 || n == 1 ? 32767 : (r * 31 + a * 17) % 23 - 4);
                                memcpy(v.at(r), old, sizeof(int16_t) * GBL_ACTIONS);
                            }
                            const int16_t *vin = drop == 2 ? nullptr : v.p;
                            const int8_t *zin = drop == 3 ? nullptr : z_in;
                            int16_t *vout = drop == 4 ? nullptr : (inplace && vin ? v.p : v2.p);
                            CHECK(gbl_cpu_reanalyse_gumbel(&ev, ci[1], 16, ci[0], noise, 50, 23, 99, (uint64_t)1 << 40, 5, o.p, po,
                                                           drop == 1 ? nullptr : m.p, pm, vin, vout, pv, zin, pz, drop == 5 ? nullptr : value.p,
                                                           drop == 6 ? nullptr : priors.p, drop == 7 ? nullptr : action.p,
                                                           drop == 8 ? nullptr : nodes.p, drop == 9 ? nullptr : moved.p,
                                                           drop == 10 ? nullptr : census.p, drop == 11 ? nullptr : gum.p, n, nullptr));
                            for (int64_t r = 0; r < n; ++r) {
                                const bool skipped = zin && r % 7 == 6;  // (its visits stay what they were: not comparable)
                                memset(visits[inplace][r], 0, sizeof visits[inplace][r]);
                                if (vout && !skipped) memcpy(visits[inplace][r], reinterpret_cast<char *>(vout) + r * pv * 2, sizeof visits[inplace][r]);
                                drift[inplace][r] = drop == 9 ? 0 : moved.p[r];
                                if (vout && vin && !skipped && drop != 9) {
                                    const int32_t want = drift_of(olds.data() + r * GBL_ACTIONS, visits[inplace][r]);
                                    if (want != moved.p[r]) {
                                        printf("drift %d, in 128 bits %d: ring %d n %lld row %lld\n", moved.p[r], want, ring, (long long)n, (long long)r);
                                        return 1;
                                    }
                                    ++drifts;
                                    int64_t So = 0, Sn = 0;
                                    for (int a = 0; a < GBL_ACTIONS; ++a) {
                                        So += olds[r * GBL_ACTIONS + a] > 0 ? olds[r * GBL_ACTIONS + a] : 0;
                                        Sn += visits[inplace][r][a];
                                    }
                                    if (2 * So * Sn > largest) largest = 2 * So * Sn;
                                }
                                sum += (uint64_t)(uint16_t)visits[inplace][r][r % GBL_ACTIONS] + (uint64_t)(uint32_t)drift[inplace][r];
                                if (drop != 5) sum += (uint64_t)(uint32_t)value.p[r];
                                if (drop != 6) sum += (uint64_t)priors.p[r * GBL_ACTIONS + r % GBL_ACTIONS];
                                if (drop != 7) sum += (uint64_t)(uint32_t)action.p[r];
                                if (drop != 8) sum += (uint64_t)(uint32_t)nodes.p[r];
                                if (drop != 10) sum += (uint64_t)(uint8_t)census.p[r];
                                if (drop != 11) sum += (uint64_t)(uint16_t)gum.p[r * GBL_ACTIONS + r % GBL_ACTIONS];
                            }
                        }
                        for (int64_t r = 0; r < n; ++r)
                            if (drift[0][r] != drift[1][r] || memcmp(visits[0][r], visits[1][r], sizeof visits[0][r]) != 0) {
                                printf("in place and separate outputs differ: ring %d n %lld rule %d/%d noise %d drop %d row %lld\n", ring,
                                       (long long)n, ci[0], ci[1], noise, drop, (long long)r);
                                return 1;
                            }
                    }
    printf("reanalyse_gumbel sanitize run: %lld drifts checked in 128 bits, largest 2 So Sn %lld, checksum %llu\n", (long long)drifts,
           (long long)largest, (unsigned long long)sum);
    return 0;
}
