// gbl_cpu_tb_targets under AddressSanitizer + UBSan, as a stand-alone program (no Python, no preload):
//   g++ -O1 -g -std=c++17 -mpopcnt -fsanitize=address,undefined -fno-omit-frame-pointer -fno-sanitize-recover=undefined -Wno-unknown-pragmas \
//       -Wno-attributes -pthread -o tb_targets_main scripts/sanitize_tb_targets_main.cpp gobblet-rl_amd/csrc/gobblet_cpu.cpp && ./tb_targets_main
// The (2, 1, 0) universe built in place, rows of its positions seen by both movers (every fifth row all zeros, every seventh with
// z = GBL_Z_OPEN), then n = 0 / 1 / 65 rows through both pitch sets -- a batch's and the ring's, z inside the mask's rows as in
// ring_meta --, in place and into outputs of their own, both modes, every optional pointer NULL in turn.  Every array is a heap block
// of EXACTLY (n - 1) * pitch + row elements, so a byte read or written beyond a row's elements is reported; the batch's arrays start at
// odd addresses.  In-place and separate outputs must agree.  Prints a checksum; any report of a sanitizer fails the run.
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

// n rows of `row` elements, `pitch` apart, in a block that ends with the last row's last element; `odd`: the block starts one byte in
template <typename T>
struct Rows {
    std::unique_ptr<char[]> block;
    T *p;
    int64_t pitch;
    Rows(int64_t n, int64_t row, int64_t pitch_, bool odd, int fill) : pitch(pitch_)
    {
        const size_t bytes = n ? ((size_t)(n - 1) * pitch + row) * sizeof(T) : 0;
        block.reset(new char[bytes + odd]);
        memset(block.get(), fill, bytes + odd);
        p = reinterpret_cast<T *>(block.get() + odd);
    }
    char *at(int64_t r) { return reinterpret_cast<char *>(p) + r * pitch * sizeof(T); }
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
    std::vector<int8_t> state(N * GBL_CELLS), to_move(N), obs(N * GBL_OBS_BYTES), legal(N * GBL_ACTIONS);
    CHECK(gbl_cpu_tb_position(inv, aux.data(), index.data(), state.data(), N, nullptr));
    for (int64_t b = 0; b < N; ++b) {
        to_move[b] = (int8_t)(b & 1);
        for (int c = 0; c < GBL_CELLS; ++c) state[b * GBL_CELLS + c] = (int8_t)(b % 5 == 4 ? 0 : (b & 1 ? -state[b * GBL_CELLS + c] : state[b * GBL_CELLS + c]));
    }
    CHECK(gbl_cpu_observe(state.data(), to_move.data(), -1, obs.data(), N, nullptr));
    CHECK(gbl_cpu_legal_mask(state.data(), to_move.data(), legal.data(), N, nullptr));
    for (int64_t b = 4; b < N; b += 5) memset(obs.data() + b * GBL_OBS_BYTES, 0, GBL_OBS_BYTES);

    uint64_t sum = 0;
    const int64_t ns[3] = {0, 1, 65};
    for (int ring = 0; ring < 2; ++ring)
        for (int64_t n : ns)
            for (int mode = 0; mode < 2; ++mode)
                for (int drop = 0; drop < 8; ++drop) {  // which optional pointer is NULL: none, mask, visits_in, z_in, visits_out, value, outcome, census
                    const int64_t po = ring ? GBL_REPLAY_OBS_PITCH : GBL_OBS_BYTES, pm = ring ? GBL_REPLAY_META_PITCH : GBL_ACTIONS,
                                  pv = ring ? GBL_REPLAY_VISITS_PITCH : GBL_ACTIONS, pz = ring ? GBL_REPLAY_META_PITCH : 1;
                    const bool odd = !ring;
                    int8_t result[2][65];
                    int16_t visits[2][65][GBL_ACTIONS];
                    for (int inplace = 0; inplace < 2; ++inplace) {
                        Rows<int8_t> o(n, GBL_OBS_BYTES, po, odd, 0x5A), m(n, ring ? GBL_REPLAY_META_Z + 1 : GBL_ACTIONS, pm, odd, 0x5A), z(n, 1, pz, odd, 0x5A),
                            z2(n, 1, pz, odd, 0x5A), value(n, 1, 1, odd, 0x5A), outcome(n, GBL_ACTIONS, GBL_ACTIONS, odd, 0x5A), census(n, 1, 1, odd, 0x5A);
                        Rows<int16_t> v(n, GBL_ACTIONS, pv, odd, 0x5A), v2(n, GBL_ACTIONS, pv, odd, 0x5A);
                        int8_t *z_in = ring ? m.p + GBL_REPLAY_META_Z : z.p;  // (the ring keeps z in byte 54 of the mask's row)
                        for (int64_t r = 0; r < n; ++r) {
                            memcpy(o.at(r), obs.data() + r * GBL_OBS_BYTES, GBL_OBS_BYTES);
                            memcpy(m.at(r), legal.data() + r * GBL_ACTIONS, GBL_ACTIONS);
                            z_in[r * pz] = (int8_t)(r % 7 == 6 ? GBL_Z_OPEN : (int)(r % 3) - 1);
                            int16_t old[GBL_ACTIONS];
                            for (int a = 0; a < GBL_ACTIONS; ++a) old[a] = (int16_t)((r * 31 + a * 17) % 23 - 4);
                            memcpy(v.at(r), old, sizeof old);
                        }
                        const int16_t *vin = drop == 2 ? nullptr : v.p;
                        const int8_t *zin = drop == 3 ? nullptr : z_in;
                        int16_t *vout = drop == 4 ? nullptr : (inplace && vin ? v.p : v2.p);
                        int8_t *zout = inplace && zin ? z_in : z2.p;
                        CHECK(gbl_cpu_tb_targets(inv, aux.data(), table.data(), o.p, po, drop == 1 ? nullptr : m.p, pm, vin, vout, pv, zin, zout, pz, mode,
                                                 mode ? 600 : 1, drop == 5 ? nullptr : value.p, drop == 6 ? nullptr : outcome.p,
                                                 drop == 7 ? nullptr : census.p, n, nullptr));
                        for (int64_t r = 0; r < n; ++r) {
                            const bool skipped = zin && zin == z_in && r % 7 == 6;  // (its output bytes stay what they were: not comparable)
                            result[inplace][r] = skipped ? 0 : zout[r * pz];
                            memset(visits[inplace][r], 0, sizeof visits[inplace][r]);
                            if (vout && !skipped) memcpy(visits[inplace][r], reinterpret_cast<char *>(vout) + r * pv * 2, sizeof visits[inplace][r]);
                            sum += (uint64_t)(uint8_t)result[inplace][r] + (uint64_t)(uint16_t)visits[inplace][r][r % GBL_ACTIONS];
                            if (drop != 5) sum += (uint64_t)(uint8_t)value.p[r];
                            if (drop != 7) sum += (uint64_t)(uint8_t)census.p[r];
                        }
                    }
                    for (int64_t r = 0; r < n; ++r)
                        if (result[0][r] != result[1][r] || memcmp(visits[0][r], visits[1][r], sizeof visits[0][r]) != 0) {
                            printf("in place and separate outputs differ: ring %d n %lld mode %d drop %d row %lld\n", ring, (long long)n, mode, drop, (long long)r);
                            return 1;
                        }
                }
    printf("tb_targets sanitize run: checksum %llu\n", (unsigned long long)sum);
    return 0;
}
