// gobblet_cpu.cpp -- the HOST flavour of the C-ABI (include/gobblet_hip.h): gbl_cpu_* with the signatures of the device entry
// points (the `stream` argument is ignored), for callers without a GPU -- BASELINE config 1 (one environment behind
// gobblet_v1.env() "on CPU"), a reference maintainer's own tests, and the CPU twin bench.py times beside the GPU (SURVEY.md 8b /
// 8d(ii)).  It is NOT a fallback: nothing in the package routes a GPU call here; a caller asks for device="cpu" explicitly.
//
// The game logic is the DEVICE code itself: this file compiles csrc/gobblet_device.h for the host (GBL_HOST_EMU selects the
// header's host paths; the handful of AMDGPU builtins it uses are given plain C++ meanings below) and walks the boards one by one
// -- row in, bit planes, the same lane functions the kernels call (legal54, play_ply, winner_of, obs_scatter_row, pick54 on the
// same Philox words, greedy_decide ...), row out.  So the twin is bit-identical to the HIP path by construction of the shared
// header and is parity-tested against the oracle like it (tests/test_cpu_twin.py).  It never includes, links or calls anything
// under oracle/.  Boards are dealt over std::threads (gbl_cpu_set_threads; default: the hardware's).
#define GBL_HOST_EMU
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#define __device__
#define __forceinline__ inline
struct uint4 {
    uint32_t x, y, z, w;
};

static inline uint32_t host_alignbyte(uint32_t hi, uint32_t lo, uint32_t n)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (n & 3u)));
}
static inline uint32_t host_udot4(uint32_t a, uint32_t b, uint32_t c, bool)
{
    for (int i = 0; i < 4; ++i) c += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
    return c;
}
static inline uint32_t host_umul24(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)(a & 0xFFFFFFu) * (b & 0xFFFFFFu)); }
static inline uint32_t host_umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
#define __builtin_amdgcn_alignbyte host_alignbyte
#define __builtin_amdgcn_udot4 host_udot4
#define __umul24 host_umul24
#define __umulhi host_umulhi
#define __popc __builtin_popcount
#define __popcll __builtin_popcountll
#define __shfl_down(v, delta) (0u)  // (row_stage's neighbour fetch: the host flavour moves rows with memcpy and never stages)

#include "gobblet_device.h"

#include "../../include/gobblet_cpu.h"

using namespace gbl;

namespace {

thread_local char g_err[256] = "";
std::atomic<int> g_threads{0};

int fail(int code, const char *msg)
{
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}

int thread_count(int64_t n, int64_t grain)
{
    int t = g_threads.load();
    if (t <= 0) t = (int)std::thread::hardware_concurrency();
    if (t <= 0) t = 1;
    const int64_t by_work = (n + grain - 1) / grain;  // a thread is worth starting for a few thousand boards (one-ply work)
    return (int)std::max<int64_t>(1, std::min<int64_t>(t, by_work));
}

// f(b0, b1) over [0, n) in contiguous ranges, one per thread; grain = boards per thread below which fewer threads start
template <typename F>
void parallel_for(int64_t n, F f, int64_t grain = 2048)
{
    const int t = thread_count(n, grain);
    if (t == 1) {
        f((int64_t)0, n);
        return;
    }
    std::vector<std::thread> pool;
    const int64_t per = (n + t - 1) / t;
    for (int i = 0; i < t; ++i) {
        const int64_t b0 = i * per, b1 = std::min(n, b0 + per);
        if (b0 < b1) pool.emplace_back([=] { f(b0, b1); });
    }
    for (auto &th : pool) th.join();
}

// a board's 27 state bytes as the seven little-endian dwords the device code works on
inline void load_row(const int8_t *state, int64_t b, uint32_t (&r)[7])
{
    r[6] = 0;
    memcpy(r, state + b * kCells, kCells);
}
inline void store_row(int8_t *state, int64_t b, const uint32_t (&r)[7]) { memcpy(state + b * kCells, r, kCells); }

struct HostRow {  // play_ply's row: the 27 bytes where they live
    uint8_t *row;
    void apply(const MoveCells &m) const
    {
        row[m.had ? m.cold : m.cnew] = 0;
        row[m.cnew] = (uint8_t)m.val;
    }
    void reset() const { memset(row, 0, kCells); }
};

inline void write_mask(int8_t *dst, uint64_t m)
{
    uint32_t d[14];
    mask_row(m, d);
    memcpy(dst, d, kActions);
}

inline void write_obs(int8_t *dst, const Planes &p, int observer)
{
    memset(dst, 0, kObs);
    obs_scatter_row(reinterpret_cast<uint8_t *>(dst), p, observer);
}

inline uint64_t read_mask(const int8_t *src)
{
    uint64_t m = 0;
    for (int a = 0; a < kActions; ++a) m |= (uint64_t)(src[a] != 0) << a;
    return m;
}

struct Tally {
    unsigned long long plies = 0, games = 0, w1 = 0, w2 = 0;
};

void add_tally(int64_t *counters, const Tally &t)  // (stripe 0: the totals are sums over the stripes)
{
    if (!counters) return;
    auto *c = reinterpret_cast<std::atomic<unsigned long long> *>(counters);
    c[0] += t.plies; c[1] += t.games; c[2] += t.w1; c[3] += t.w2;
}

inline int64_t cell_of(int64_t b, uint32_t t, int64_t ply_stride, int64_t tile_stride)
{
    return (int64_t)t * ply_stride + (b / kTile) * tile_stride + (b % kTile);
}

inline uint32_t hist_prev3(const int8_t *hist, int64_t b, int me)
{
    if (!hist) return 0x00FFFFFFu;
    const uint8_t *h = reinterpret_cast<const uint8_t *>(hist) + (b * 2 + me) * 3;
    return (uint32_t)h[0] | ((uint32_t)h[1] << 8) | ((uint32_t)h[2] << 16);
}

}  // namespace

extern "C" {

const char *gbl_cpu_last_error(void) { return g_err; }

int gbl_cpu_set_threads(int threads)  // 0 = the hardware's (host flavour only)
{
    if (threads < 0) return fail(GBL_ERR_ARG, "threads < 0");
    g_threads.store(threads);
    return GBL_OK;
}

int gbl_cpu_layout_info(int32_t out[6])
{
    if (!out) return fail(GBL_ERR_ARG, "out must not be NULL");
    out[0] = GBL_ABI_VERSION; out[1] = kCells; out[2] = kActions; out[3] = kObs; out[4] = kTile; out[5] = 1;  // (no alignment asked of host buffers)
    return GBL_OK;
}

int gbl_cpu_reset(int8_t *state, int8_t *to_move, int8_t *done, int8_t *winner, int64_t n, void *)
{
    if (const char *why = reset_error(n, state, to_move, done)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    memset(state, 0, (size_t)n * kCells);
    memset(to_move, 0, (size_t)n);
    memset(done, 0, (size_t)n);
    if (winner) memset(winner, 0, (size_t)n);
    return GBL_OK;
}

int gbl_cpu_legal_mask(const int8_t *state, const int8_t *to_move, int8_t *mask, int64_t n, void *)
{
    if (const char *why = legal_mask_error(n, state, to_move, mask)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) {
            uint32_t r[7];
            load_row(state, b, r);
            write_mask(mask + b * kActions, legal54(make_planes(r), to_move[b] != 0));
        }
    });
    return GBL_OK;
}

int gbl_cpu_is_legal(const int8_t *state, const int8_t *agent_index, const int32_t *actions, int8_t *out, int64_t n, void *)
{
    if (const char *why = is_legal_error(n, state, agent_index, actions, out)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    for (int64_t b = 0; b < n; ++b) {
        uint32_t r[7];
        load_row(state, b, r);
        const int a = actions[b];
        const uint64_t m = legal54(make_planes(r), agent_index[b] != 0);
        out[b] = ((uint32_t)a < (uint32_t)kActions && ((m >> (a & 63)) & 1ull)) ? 1 : 0;
    }
    return GBL_OK;
}

int gbl_cpu_play_turn(int8_t *state, const int8_t *agent_index, const int32_t *actions, int64_t n, void *)
{
    if (const char *why = play_turn_error(n, state, agent_index, actions)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    for (int64_t b = 0; b < n; ++b) {
        uint32_t r[7];
        load_row(state, b, r);
        Planes p = make_planes(r);
        const int a = actions[b], mover = agent_index[b] != 0;
        const uint64_t m = legal54(p, mover);
        if ((uint32_t)a < (uint32_t)kActions && ((m >> (a & 63)) & 1ull)) {
            apply_move(p, r, mover, (uint32_t)a);
            store_row(state, b, r);
        }
    }
    return GBL_OK;
}

int gbl_cpu_winner(const int8_t *state, int8_t *winner, int64_t n, void *)
{
    if (const char *why = winner_error(n, state, winner)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    for (int64_t b = 0; b < n; ++b) {
        uint32_t r[7];
        load_row(state, b, r);
        winner[b] = (int8_t)winner_of(make_planes(r));
    }
    return GBL_OK;
}

int gbl_cpu_flatboard(const int8_t *state, int8_t *flat, int64_t n, void *)
{
    if (const char *why = flatboard_error(n, state, flat)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    for (int64_t b = 0; b < n; ++b) {
        uint32_t r[7], d[3];
        load_row(state, b, r);
        flat_row(make_planes(r), r, d);
        memcpy(flat + b * 9, d, 9);
    }
    return GBL_OK;
}

int gbl_cpu_covered(const int8_t *state, int8_t *cov, int64_t n, void *)
{
    if (const char *why = covered_error(n, state, cov)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    for (int64_t b = 0; b < n; ++b) {
        uint32_t r[7], d[7];
        load_row(state, b, r);
        covered_row(make_planes(r), d);
        memcpy(cov + b * kCells, d, kCells);
    }
    return GBL_OK;
}

int gbl_cpu_validate(const int8_t *state, int8_t *flags, int64_t n, void *)
{
    if (const char *why = validate_error(n, state, flags)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    for (int64_t b = 0; b < n; ++b) {
        uint32_t r[7];
        load_row(state, b, r);
        flags[b] = (int8_t)validate_row(r);
    }
    return GBL_OK;
}

int gbl_cpu_observe(const int8_t *state, const int8_t *to_move, int agent_sel, int8_t *obs, int64_t n, void *)
{
    if (const char *why = observe_error(n, state, to_move, agent_sel, obs)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) {
            uint32_t r[7];
            load_row(state, b, r);
            const int who = agent_sel >= 0 ? agent_sel : to_move[b];
            write_obs(obs + b * kObs, make_planes(r), who != 0);
        }
    });
    return GBL_OK;
}

int gbl_cpu_board_eval(int8_t *state, const int8_t *agent_index, const int32_t *actions, int8_t *record_out, int64_t n, void *)
{
    if (const char *why = board_eval_error(n, state, agent_index, actions, record_out)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    for (int64_t b = 0; b < n; ++b) {
        uint32_t r[7];
        load_row(state, b, r);
        Planes p = make_planes(r);
        if (actions) {  // board.py:118-132
            const int a = actions[b], mover = agent_index[b] != 0;
            const uint64_t m = legal54(p, mover);
            if ((uint32_t)a < (uint32_t)kActions && ((m >> (a & 63)) & 1ull)) apply_move(p, r, mover, (uint32_t)a);
            store_row(state, b, r);
        }
        int8_t *rec = record_out + b * GBL_REC_BYTES;
        memset(rec, 0, GBL_REC_BYTES);
        memcpy(rec + GBL_REC_SQUARES, r, kCells);
        rec[GBL_REC_WINNER] = (int8_t)winner_of(p);
        uint32_t f[3], c[7];
        flat_row(p, r, f);
        covered_row(p, c);
        memcpy(rec + GBL_REC_FLAT, f, 9);
        memcpy(rec + GBL_REC_COVERED, c, kCells);
        write_mask(rec + GBL_REC_MASK0, legal54(p, 0));
        write_mask(rec + GBL_REC_MASK1, legal54(p, 1));
        obs_scatter_row(reinterpret_cast<uint8_t *>(rec) + GBL_REC_OBS0, p, 0);
        obs_scatter_row(reinterpret_cast<uint8_t *>(rec) + GBL_REC_OBS1, p, 1);
    }
    return GBL_OK;
}

int gbl_cpu_step_ex(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *actions, int8_t *winner_out, int8_t *reward_out,
                    int8_t *mask_out, int8_t *obs_out, int32_t *turn, int32_t *actions_out, int8_t *done_out, int8_t *to_move_out,
                    int8_t *status_out, int32_t *next_actions_out, uint64_t seed, uint64_t env_base, uint32_t ply,
                    const uint32_t *ply_dev, int64_t n, int illegal_mode, int auto_reset, void *)
{
    if (const char *why = step_error(n, state, to_move, done, actions, illegal_mode)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    auto_reset = auto_reset != 0;
    if (ply_dev) ply += *ply_dev;
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) {
            uint32_t r[7];
            load_row(state, b, r);
            Planes p = make_planes(r);
            int mover = to_move[b] != 0;
            const int was_done = !auto_reset && done[b] != 0, action = actions[b];
            Ply y;
            int dn;
            step_lane(HostRow{reinterpret_cast<uint8_t *>(state) + b * kCells}, p, mover, was_done, action, illegal_mode, auto_reset, dn, y);
            to_move[b] = (int8_t)mover;
            done[b] = (int8_t)dn;
            if (winner_out) winner_out[b] = (int8_t)y.winner;
            if (reward_out) { reward_out[2 * b] = (int8_t)y.r0; reward_out[2 * b + 1] = (int8_t)y.r1; }
            if (turn) turn[b] = next_turn(turn[b], y, auto_reset);
            if (obs_out) write_obs(obs_out + b * kObs, p, mover);
            const uint64_t legal = next_mask(p, mover, dn, auto_reset);
            if (mask_out) write_mask(mask_out + b * kActions, legal);
            if (actions_out) actions_out[b] = action;
            if (done_out) done_out[b] = (int8_t)dn;
            if (to_move_out) to_move_out[b] = (int8_t)mover;
            if (status_out) status_out[b] = (int8_t)(was_done ? 0 : action_status(y.ok, action));  // (a frozen board consumes no action)
            if (next_actions_out) next_actions_out[b] = sample54(legal, seed, env_base + (uint64_t)b, ply);  // (may alias `actions`)
        }
    });
    return GBL_OK;
}

int gbl_cpu_sample_at(const int8_t *mask, int32_t *actions, int64_t n, uint64_t seed, uint64_t env_base, uint32_t ply,
                      const uint32_t *ply_dev, void *)
{
    if (const char *why = sample_error(n, mask, actions)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    if (ply_dev) ply += *ply_dev;
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) actions[b] = sample54(read_mask(mask + b * kActions), seed, env_base + (uint64_t)b, ply);
    });
    return GBL_OK;
}

int gbl_cpu_counter_add(uint32_t *counter, uint32_t by, void *)
{
    if (!counter) return fail(GBL_ERR_ARG, "counter must not be NULL");
    *counter += by;
    return GBL_OK;
}

// the masked-random ply of one board (sample -> step -> auto-reset), shared by rollout / collect
static inline Ply random_ply(Planes &p, HostRow row, int &mover, uint64_t &legal, int &action, int given, bool use_given, uint64_t seed,
                             uint64_t id, uint32_t ply, int illegal_mode, int &dn)
{
    action = use_given ? given : sample54(legal, seed, id, ply);
    Ply y = play_ply(p, row, mover, legal, action, illegal_mode);
    dn = y.terminal ? 1 : 0;
    if (y.terminal) {  // raw_env.reset, gobblet.py:275-290
        p = Planes{0u, 0u, 0u};
        mover = 0;
        row.reset();
    }
    legal = legal54(p, mover);
    return y;
}

int gbl_cpu_rollout_at(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_out, int8_t *winner_out, int8_t *reward_out,
                       int8_t *mask_out, int8_t *obs_out, int64_t n, uint64_t seed, uint64_t env_base, uint32_t ply0,
                       const uint32_t *ply_dev, uint32_t plies, int illegal_mode, int64_t *counters, int32_t *turn, void *)
{
    if (const char *why = rollout_error(n, state, to_move, done, illegal_mode)) return fail(GBL_ERR_ARG, why);
    if (n == 0 || plies == 0) return GBL_OK;
    if (ply_dev) ply0 += *ply_dev;
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        Tally tl;
        for (int64_t b = b0; b < b1; ++b) {
            uint32_t r[7];
            load_row(state, b, r);
            Planes p = make_planes(r);
            const HostRow row{reinterpret_cast<uint8_t *>(state) + b * kCells};
            int mover = to_move[b] != 0, dn = 0, action = -1, tcount = 0;
            bool treset = false;
            uint64_t legal = legal54(p, mover);
            Ply y{0, 0, 0, false, false};
            for (uint32_t t = 0; t < plies; ++t) {
                y = random_ply(p, row, mover, legal, action, 0, false, seed, env_base + (uint64_t)b, ply0 + t, illegal_mode, dn);
                tcount = next_turn(tcount, y, 1);
                treset = treset || y.terminal;
                tl.games += y.terminal; tl.w1 += y.winner == 1; tl.w2 += y.winner == -1;
            }
            tl.plies += plies;
            to_move[b] = (int8_t)mover;
            done[b] = (int8_t)dn;
            if (actions_out) actions_out[b] = action;
            if (winner_out) winner_out[b] = (int8_t)y.winner;
            if (reward_out) { reward_out[2 * b] = (int8_t)y.r0; reward_out[2 * b + 1] = (int8_t)y.r1; }
            if (turn) turn[b] = treset ? tcount : turn[b] + tcount;
            if (obs_out) write_obs(obs_out + b * kObs, p, mover);
            if (mask_out) write_mask(mask_out + b * kActions, legal);
        }
        add_tally(counters, tl);
    });
    return GBL_OK;
}

int gbl_cpu_collect_from_ex(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *first_actions, int8_t *first_status,
                            int32_t *actions_traj, int8_t *winner_traj, int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj,
                            int8_t *mask_traj, int8_t *obs_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed,
                            uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int illegal_mode,
                            int64_t *counters, int32_t *turn, void *)
{
    if (const char *why = collect_error(n, first_actions, first_status, state, to_move, done, illegal_mode, plies, ply_stride, tile_stride))
        return fail(GBL_ERR_ARG, why);
    if (n == 0 || plies == 0) return GBL_OK;
    if (ply_dev) ply0 += *ply_dev;
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        Tally tl;
        for (int64_t b = b0; b < b1; ++b) {
            uint32_t r[7];
            load_row(state, b, r);
            Planes p = make_planes(r);
            const HostRow row{reinterpret_cast<uint8_t *>(state) + b * kCells};
            int mover = to_move[b] != 0, dn = 0, action = -1, tcount = 0;
            bool treset = false;
            uint64_t legal = legal54(p, mover);
            for (uint32_t t = 0; t < plies; ++t) {
                const bool given = first_actions && t == 0;
                const Ply y = random_ply(p, row, mover, legal, action, given ? first_actions[b] : 0, given, seed, env_base + (uint64_t)b,
                                         ply0 + t, illegal_mode, dn);
                if (given && first_status) first_status[b] = (int8_t)action_status(y.ok, action);
                tcount = next_turn(tcount, y, 1);
                treset = treset || y.terminal;
                tl.games += y.terminal; tl.w1 += y.winner == 1; tl.w2 += y.winner == -1;
                const int64_t at = cell_of(b, t, ply_stride, tile_stride);
                if (actions_traj) actions_traj[at] = action;
                if (winner_traj) winner_traj[at] = (int8_t)y.winner;
                if (reward_traj) { reward_traj[2 * at] = (int8_t)y.r0; reward_traj[2 * at + 1] = (int8_t)y.r1; }
                if (done_traj) done_traj[at] = (int8_t)dn;
                if (to_move_traj) to_move_traj[at] = (int8_t)mover;
                if (obs_traj) write_obs(obs_traj + at * kObs, p, mover);
                if (mask_traj) write_mask(mask_traj + at * kActions, legal);
            }
            tl.plies += plies;
            to_move[b] = (int8_t)mover;
            done[b] = (int8_t)dn;
            if (turn) turn[b] = treset ? tcount : turn[b] + tcount;
        }
        add_tally(counters, tl);
    });
    return GBL_OK;
}

int gbl_cpu_decode_obs(const int8_t *obs, int8_t *state, int8_t *to_move, int64_t n, void *)
{
    if (const char *why = decode_obs_error(n, obs, state, to_move)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    for (int64_t b = 0; b < n; ++b) {
        uint32_t d[30], r[7];
        d[29] = 0;
        memcpy(d, obs + b * kObs, kObs);
        to_move[b] = (int8_t)decode_obs_row(d, r);
        store_row(state, b, r);
    }
    return GBL_OK;
}

// one decision: chosen-before-fallback / candidate set / fallback flag (gbl_greedy), and with hist_rw the returned action and the
// history append (gbl_greedy_act)
static int greedy_run(const int8_t *state, const int8_t *to_move, const int8_t *mask, const int8_t *hist, int depth, int32_t *action_out,
                      int8_t *cand_out, int8_t *fallback_out, int64_t n, int8_t *hist_rw, int32_t *final_out, uint64_t seed,
                      uint64_t env_base, uint32_t call)
{
    if (hist_rw) hist = hist_rw;
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) {
            uint32_t r[7];
            load_row(state, b, r);
            const Planes p = make_planes(r);
            const int me = to_move[b] != 0;
            const uint64_t m = mask ? read_mask(mask + b * kActions) : legal54(p, me);
            const uint32_t prev3 = hist_prev3(hist, b, me);
            const GreedyResult g = greedy_decide(p, me, m, depth, prev3);
            if (action_out) action_out[b] = g.fallback ? -1 : g.chosen;
            if (fallback_out) fallback_out[b] = g.fallback ? 1 : 0;
            if (cand_out) write_mask(cand_out + b * kActions, g.cands);
            if (hist_rw) {  // :211-217 with the library's sampler, then :219
                const int fin = g.fallback ? pick54(g.cands, draw32(seed, env_base + (uint64_t)b, call, kStreamGreedy)) : g.chosen;
                final_out[b] = fin;
                int8_t *hp = hist_rw + (b * 2 + me) * 3;
                hp[0] = (int8_t)(prev3 >> 8);
                hp[1] = (int8_t)(prev3 >> 16);
                hp[2] = (int8_t)fin;
            }
        }
    });
    return GBL_OK;
}

int gbl_cpu_greedy(const int8_t *state, const int8_t *to_move, const int8_t *mask, const int8_t *hist, int depth, int32_t *action_out,
                   int8_t *cand_mask_out, int8_t *fallback_out, int64_t n, void *)
{
    if (const char *why = greedy_error(n, state, to_move, action_out, depth)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    return greedy_run(state, to_move, mask, hist, depth, action_out, cand_mask_out, fallback_out, n, nullptr, nullptr, 0, 0, 0);
}

int gbl_cpu_greedy_act_at(const int8_t *state, const int8_t *to_move, const int8_t *mask, int8_t *hist, int depth, uint64_t seed,
                          uint64_t env_base, uint32_t call, const uint32_t *call_dev, int32_t *action_out, int32_t *chosen_out,
                          int8_t *cand_mask_out, int8_t *fallback_out, int64_t n, void *)
{
    if (const char *why = greedy_act_error(n, state, to_move, hist, action_out, depth)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    if (call_dev) call += *call_dev;
    return greedy_run(state, to_move, mask, nullptr, depth, chosen_out, cand_mask_out, fallback_out, n, hist, action_out, seed, env_base,
                      call);
}

// Board b as the search entry points (gbl_cpu_playout_values, _tree_search, _evaluate, _tree_search_eval) take it: its planes, the
// mover and the candidates -- the mover's legal actions, less those whose byte of the board's `mask` row (optional) is zero
struct HostRoot {
    Planes p;
    int mover;
    uint64_t cand;
};

static HostRoot host_root(const int8_t *state, const int8_t *to_move, const int8_t *mask, int64_t b)
{
    uint32_t r[7];
    load_row(state, b, r);
    HostRoot R{make_planes(r), to_move[b] != 0, 0};
    R.cand = legal54(R.p, R.mover);
    if (mask) R.cand &= read_mask(mask + b * kActions);
    return R;
}

int gbl_cpu_playout_values(const int8_t *state, const int8_t *to_move, const int8_t *mask, int playouts, int max_plies,
                           uint64_t seed, uint64_t env_base, uint32_t call, int32_t *wins_out, int32_t *losses_out,
                           int32_t *action_out, int32_t *plies_out, int64_t n, void *)
{
    if (const char *why = playout_values_error(playouts, max_plies, call, env_base, n, state, to_move)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    parallel_for(n, [=](int64_t b0, int64_t b1) {  // (a board is playouts x ~30 whole games: every board is worth a thread)
        for (int64_t b = b0; b < b1; ++b) {
            const HostRoot R = host_root(state, to_move, mask, b);
            int32_t wins[kActions] = {}, losses[kActions] = {};
            uint32_t plies = 0, best = 0;
            for (int a = 0; a < kActions; ++a) {
                if (!((R.cand >> a) & 1ull)) continue;
                for (int k = 0; k < playouts; ++k) {
                    const PlayoutEnd e = playout(R.p, R.mover, a, seed, playout_id(env_base + (uint64_t)b, (uint32_t)a, (uint32_t)k), call,
                                                 (uint32_t)max_plies);
                    wins[a] += e.outcome > 0;
                    losses[a] += e.outcome < 0;
                    plies += e.plies;
                }
                best = std::max(best, playout_key(wins[a], losses[a], a));
            }
            if (wins_out) memcpy(wins_out + b * kActions, wins, sizeof wins);
            if (losses_out) memcpy(losses_out + b * kActions, losses, sizeof losses);
            if (action_out) action_out[b] = playout_action_of(best);
            if (plies_out) plies_out[b] = (int32_t)plies;
        }
    }, 1);
    return GBL_OK;
}

// One board's solve (the contract of gbl_solve): the 54 result bytes into out, the decision's key back (solve_action_of /
// solve_value_of read it)
static uint32_t host_solve(const Planes &p, int mover, uint64_t cand, int depth, int8_t (&out)[kActions])
{
    uint32_t best = 0;
    for (uint32_t a = 0; a < (uint32_t)kActions; ++a) {
        out[a] = (int8_t)kSolveNone;
        if (!((cand >> a) & 1ull)) continue;
        SolveRoot A = solve_root_action(p, mover, a, depth);
        for (uint64_t l = A.deep; l; l &= l - 1)
            A.key = std::max(A.key, solve_reply(p, mover, a, (uint32_t)__builtin_ctzll(l), depth, A.key));
        if (A.deep) A.c = solve_parent(solve_of_key(A.key));
        out[a] = (int8_t)A.c;
        best = std::max(best, solve_action_key(A.c, a));
    }
    return best;
}

int gbl_cpu_solve(const int8_t *state, const int8_t *to_move, const int8_t *mask, int depth, int8_t *outcome_out, int8_t *value_out,
                  int32_t *action_out, int64_t n, void *)
{
    int code = 0;
    if (const char *why = solve_error(depth, n, state, to_move, action_out, code)) return fail(code ? GBL_ERR_ALIGN : GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    parallel_for(n, [=](int64_t b0, int64_t b1) {  // (a board is a whole game tree: every board is worth a thread)
        for (int64_t b = b0; b < b1; ++b) {
            const HostRoot R = host_root(state, to_move, mask, b);
            int8_t out[kActions];
            const uint32_t best = host_solve(R.p, R.mover, R.cand, depth, out);
            if (outcome_out) memcpy(outcome_out + b * kActions, out, sizeof out);
            if (value_out) value_out[b] = (int8_t)solve_value_of(best);
            if (action_out) action_out[b] = solve_action_of(best);
        }
    }, 1);
    return GBL_OK;
}

// One board's search (the contract of gbl_tree_search, one iteration and one playout at a time): the root's children into visits /
// wins / losses (zeroed here), the decision's order key (0: no child), the nodes created and the plies played.
struct HostSearch {
    int32_t visits[kActions], wins[kActions], losses[kActions];
    uint64_t best;
    uint32_t count, plies;
};

// The read-out of a finished search, for both host searches: the root's children into the three rows and the decision's key
static void host_root_out(const std::vector<TreeNode> &nodes, uint32_t count, HostSearch &out)
{
    memset(out.visits, 0, sizeof out.visits); memset(out.wins, 0, sizeof out.wins); memset(out.losses, 0, sizeof out.losses);
    out.best = 0;
    for (uint32_t c = nodes[0].child; c; c = nodes[c].sibling) {
        const TreeNode &k = nodes[c];
        const uint32_t a = tree_action(k);
        out.visits[a] = k.n; out.wins[a] = (int32_t)tree_wins(k); out.losses[a] = (int32_t)tree_losses(k);
        out.best = std::max(out.best, tree_final_key(k.n, tree_wins(k), tree_losses(k), a));
    }
    out.count = count;
}

// ... and its write-out into board b's rows of an entry point's outputs, each only if its pointer is given
static void host_search_out(const HostSearch &h, int64_t b, int32_t *visits_out, int32_t *wins_out, int32_t *losses_out, int32_t *action_out,
                            int32_t *nodes_out)
{
    if (visits_out) memcpy(visits_out + b * kActions, h.visits, sizeof h.visits);
    if (wins_out) memcpy(wins_out + b * kActions, h.wins, sizeof h.wins);
    if (losses_out) memcpy(losses_out + b * kActions, h.losses, sizeof h.losses);
    if (action_out) action_out[b] = tree_action_of(h.best);
    if (nodes_out) nodes_out[b] = (int32_t)h.count;
}

static void host_tree_search(std::vector<TreeNode> &nodes, const Planes &root, int mover, uint64_t cand, uint64_t g, uint32_t iterations,
                             uint32_t P, uint32_t max_plies, uint32_t explore, uint64_t seed, uint32_t call, HostSearch &out)
{
    nodes[0] = TreeNode{};
    uint32_t count = 1, plies = 0;
    for (uint32_t i = 0; cand && i < iterations; ++i) {
        TreeLeaf s = tree_select(nodes.data(), root, mover, cand, P, explore);
        const uint32_t parent = s.node;
        uint32_t term = tree_term(nodes[s.node]), a = 0;
        const bool grow = s.untried != 0;
        if (grow) a = tree_expand_move(s.p, s.side, s.untried, draw32(seed, tree_pid(g, i, 0), playout_ply_index(call, 0), kStreamTree), term);
        uint32_t wl = tree_decided(term, P);
        for (uint32_t j = 0; term == kTreeOpen && j < P; ++j) {
            const PlayoutEnd e = tree_playout(s.p, s.side, seed, tree_pid(g, i, j), call, max_plies);
            wl += e.outcome > 0 ? 1u : (e.outcome < 0 ? 1u << 16 : 0u);
            plies += e.plies;
        }
        if (grow) tree_link(nodes.data(), s.node = count++, parent, a, term);
        tree_backup(nodes.data(), s.node, wl & 0xFFFFu, wl >> 16);
    }
    host_root_out(nodes, count, out);
    out.plies = plies;
}

int gbl_cpu_tree_search(const int8_t *state, const int8_t *to_move, const int8_t *mask, int iterations, int playouts, int max_plies,
                        int explore, uint64_t seed, uint64_t env_base, uint32_t call, int32_t *visits_out, int32_t *wins_out,
                        int32_t *losses_out, int32_t *action_out, int32_t *nodes_out, int32_t *plies_out, int64_t n, void *)
{
    if (const char *why = tree_search_error(iterations, playouts, max_plies, explore, call, env_base, n, state, to_move))
        return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    parallel_for(n, [=](int64_t b0, int64_t b1) {  // (a board is a whole search: every board is worth a thread)
        std::vector<TreeNode> nodes((size_t)iterations + 1);
        HostSearch h;
        for (int64_t b = b0; b < b1; ++b) {
            const HostRoot R = host_root(state, to_move, mask, b);
            host_tree_search(nodes, R.p, R.mover, R.cand, env_base + (uint64_t)b, (uint32_t)iterations, (uint32_t)playouts, (uint32_t)max_plies,
                             (uint32_t)explore, seed, call, h);
            host_search_out(h, b, visits_out, wins_out, losses_out, action_out, nodes_out);
            if (plies_out) plies_out[b] = (int32_t)h.plies;
        }
    }, 1);
    return GBL_OK;
}

// gbl_evaluator as the shared functions take it
static inline EvalNet eval_net(const gbl_evaluator *ev)
{
    return EvalNet{ev->w1, ev->b1, ev->w2, ev->b2, ev->hidden, ev->shift1, ev->shift_p, ev->shift_v};
}

// One evaluation (the contract of gbl_evaluate): the outputs, the prior row over `cand` (zeros where it is empty) and q.
static int32_t host_evaluate(const EvalNet &net, const Planes &p, int side, uint64_t cand, uint8_t *pri, int32_t (&o)[kEvalOutputs])
{
    uint32_t h4[kEvalMaxHidden / 4];
    eval_hidden(net, p, side, h4);
    eval_outputs(net, h4, o);
    if (cand)
        eval_priors(net, o, cand, pri);
    else
        memset(pri, 0, kActions);
    return eval_value(net, o[kEvalValue]);
}

int gbl_cpu_evaluate(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, uint8_t *priors_out,
                     int32_t *value_out, int32_t *logits_out, int64_t n, void *)
{
    if (const char *why = evaluate_error(ev, n, state, to_move, priors_out, value_out)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    const EvalNet net = eval_net(ev);
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) {
            const HostRoot R = host_root(state, to_move, mask, b);
            int32_t o[kEvalOutputs];
            value_out[b] = host_evaluate(net, R.p, R.mover, R.cand, priors_out + b * kActions, o);
            if (logits_out) memcpy(logits_out + b * kEvalOutputs, o, sizeof o);
        }
    }, 256);
    return GBL_OK;
}

// One board's evaluator-guided search (the contract of gbl_tree_search_eval, one iteration at a time): HostSearch as
// host_tree_search, and the root's q; pri[0 .. 53] is the row the root keeps (pi' where there is noise, else the network's row).
struct HostNoise {  // the root noise of one search (w == 0: none); root_pi: where the network's row goes (NULL: nowhere)
    uint32_t w;
    uint64_t seed, g;
    uint32_t q;
    uint8_t *root_pi;
};

// The Gumbel root rule of one search (G.considered == 0: none, the root selects by its keys): in, the rule's arguments and the
// generator's (seed, g, q); out, the decision, the target row and the g row (zeros outside the candidates).
struct HostGumbel {
    GumbelArgs G;
    uint64_t seed, g;
    uint32_t q;
    int action;
    uint8_t target[kActions];
    int16_t gum[kActions];
};

static int32_t host_tree_search_eval(std::vector<TreeNode> &nodes, std::vector<uint8_t> &pri, const EvalNet &net, const Planes &root,
                                     int mover, uint64_t cand, uint32_t iterations, uint32_t explore, HostSearch &out,
                                     const HostNoise &noise = HostNoise{}, HostGumbel *gumbel = nullptr)
{
    int32_t o[kEvalOutputs];
    nodes[0] = TreeNode{};
    const int32_t root_q = host_evaluate(net, root, mover, cand, pri.data(), o);
    if (noise.root_pi) memcpy(noise.root_pi, pri.data(), kActions);
    if (noise.w && cand) noise_priors(noise.seed, noise.g, noise.q, noise.w, cand, pri.data(), pri.data());
    GumbelRoot R;
    const bool rule = gumbel && gumbel->G.considered && cand;
    if (rule) gumbel_root_init(R, gumbel->G, iterations, gumbel->seed, gumbel->g, gumbel->q, cand, o, net.shift_p, root_q);
    uint32_t count = 1;
    for (uint32_t i = 0; cand && i < iterations; ++i) {
        TreeEvalLeaf s = tree_eval_select(nodes.data(), pri.data(), root, mover, cand, explore, rule ? gumbel_root_select(R, nodes.data()) : -1);
        uint32_t term = tree_term(nodes[s.node]);
        if (s.expand) {
            term = tree_move_into(s.p, s.side, s.a);
            tree_link(nodes.data(), count, s.node, s.a, term);
            s.node = count++;
        }
        uint32_t wl = tree_decided(term, kTreeEvalP);
        if (s.expand && term == kTreeOpen)
            wl = tree_eval_outcome(host_evaluate(net, s.p, s.side, legal54(s.p, s.side), pri.data() + (size_t)s.node * kEvalOutputs, o));
        tree_backup(nodes.data(), s.node, wl & 0xFFFFu, wl >> 16);
    }
    host_root_out(nodes, count, out);
    out.plies = 0;
    if (gumbel) {
        gumbel->action = -1;
        memset(gumbel->target, 0, sizeof gumbel->target);
        memset(gumbel->gum, 0, sizeof gumbel->gum);
        if (rule) {
            gumbel->action = gumbel_root_finish(R, nodes.data(), gumbel->target);
            for (int a = 0; a < kActions; ++a) gumbel->gum[a] = (int16_t)R.gum[a];
        }
    }
    return root_q;
}

static int host_tree_search_eval_run(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                                     int explore, int noise, uint64_t seed, uint64_t env_base, uint32_t call, int32_t *visits_out,
                                     int32_t *wins_out, int32_t *losses_out, int32_t *action_out, int32_t *nodes_out,
                                     int32_t *root_value_out, uint8_t *root_priors_out, uint8_t *root_mixed_out, int64_t n)
{
    if (const char *why = tree_search_eval_error(ev, iterations, explore, n, state, to_move)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    const EvalNet net = eval_net(ev);
    parallel_for(n, [=](int64_t b0, int64_t b1) {  // (a board is a whole search: every board is worth a thread)
        std::vector<TreeNode> nodes((size_t)iterations + 1);
        std::vector<uint8_t> pri(((size_t)iterations + 1) * kEvalOutputs);
        HostSearch h;
        for (int64_t b = b0; b < b1; ++b) {
            const HostRoot R = host_root(state, to_move, mask, b);
            const int32_t q = host_tree_search_eval(nodes, pri, net, R.p, R.mover, R.cand, (uint32_t)iterations, (uint32_t)explore, h,
                                                    HostNoise{(uint32_t)noise, seed, env_base + (uint64_t)b, call,
                                                              root_priors_out ? root_priors_out + b * kActions : nullptr});
            host_search_out(h, b, visits_out, wins_out, losses_out, action_out, nodes_out);
            if (root_value_out) root_value_out[b] = q;
            if (root_mixed_out) memcpy(root_mixed_out + b * kActions, pri.data(), kActions);
        }
    }, 1);
    return GBL_OK;
}

int gbl_cpu_tree_search_eval(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                             int explore, int32_t *visits_out, int32_t *wins_out, int32_t *losses_out, int32_t *action_out,
                             int32_t *nodes_out, int32_t *root_value_out, uint8_t *root_priors_out, int64_t n, void *)
{
    return host_tree_search_eval_run(state, to_move, mask, ev, iterations, explore, 0, 0, 0, 0, visits_out, wins_out, losses_out, action_out,
                                     nodes_out, root_value_out, root_priors_out, nullptr, n);
}

int gbl_cpu_tree_search_eval_noise(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                                   int explore, int noise, uint64_t seed, uint64_t env_base, uint32_t call, int32_t *visits_out,
                                   int32_t *wins_out, int32_t *losses_out, int32_t *action_out, int32_t *nodes_out,
                                   int32_t *root_value_out, uint8_t *root_priors_out, uint8_t *root_mixed_out, int64_t n, void *)
{
    if (const char *why = tree_search_noise_error(noise, call, env_base, n)) return fail(GBL_ERR_ARG, why);
    return host_tree_search_eval_run(state, to_move, mask, ev, iterations, explore, noise, seed, env_base, call, visits_out, wins_out,
                                     losses_out, action_out, nodes_out, root_value_out, root_priors_out, root_mixed_out, n);
}

int gbl_cpu_tree_search_gumbel(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                               int explore, int considered, int gumbel_noise, int visit_offset, int scale, uint64_t seed,
                               uint64_t env_base, uint32_t call, int32_t *visits_out, int32_t *wins_out, int32_t *losses_out,
                               int32_t *action_out, int32_t *nodes_out, int32_t *root_value_out, uint8_t *root_priors_out,
                               uint8_t *target_out, int16_t *gumbel_out, int64_t n, void *)
{
    if (const char *why = tree_search_gumbel_error(ev, iterations, explore, considered, gumbel_noise, visit_offset, scale, call, env_base, n,
                                                   state, to_move))
        return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    const EvalNet net = eval_net(ev);
    const GumbelArgs G{(uint32_t)considered, (uint32_t)gumbel_noise, (uint32_t)visit_offset, (uint32_t)scale};
    parallel_for(n, [=](int64_t b0, int64_t b1) {  // (a board is a whole search: every board is worth a thread)
        std::vector<TreeNode> nodes((size_t)iterations + 1);
        std::vector<uint8_t> pri(((size_t)iterations + 1) * kEvalOutputs);
        HostSearch h;
        HostGumbel gb{G, seed, 0, call, -1, {}, {}};
        for (int64_t b = b0; b < b1; ++b) {
            const HostRoot R = host_root(state, to_move, mask, b);
            gb.g = env_base + (uint64_t)b;
            const int32_t q = host_tree_search_eval(nodes, pri, net, R.p, R.mover, R.cand, (uint32_t)iterations, (uint32_t)explore, h,
                                                    HostNoise{0, 0, 0, 0, root_priors_out ? root_priors_out + b * kActions : nullptr}, &gb);
            host_search_out(h, b, visits_out, wins_out, losses_out, nullptr, nodes_out);
            if (action_out) action_out[b] = gb.action;
            if (root_value_out) root_value_out[b] = q;
            if (target_out) memcpy(target_out + b * kActions, gb.target, sizeof gb.target);
            if (gumbel_out) memcpy(gumbel_out + b * kActions, gb.gum, sizeof gb.gum);
        }
    }, 1);
    return GBL_OK;
}

int gbl_cpu_collect_policy(int8_t *state, int8_t *to_move, int8_t *done, int8_t *hist, int32_t *actions_traj, int8_t *winner_traj,
                           int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                           int32_t *chosen_traj, int8_t *how_traj, int8_t *cand_traj, int64_t n, int64_t ply_stride,
                           int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev,
                           uint32_t plies, int policy0, int policy1, int opening_plies, int illegal_mode, int64_t *counters,
                           int32_t *turn, void *)
{
    if (const char *why = collect_policy_error(n, state, to_move, done, illegal_mode, policy0, policy1, opening_plies, turn != nullptr, plies,
                                                 ply_stride, tile_stride))
        return fail(GBL_ERR_ARG, why);
    if (n == 0 || plies == 0) return GBL_OK;
    if (ply_dev) ply0 += *ply_dev;
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        Tally tl;
        for (int64_t b = b0; b < b1; ++b) {
            uint32_t r[7];
            load_row(state, b, r);
            Planes p = make_planes(r);
            const HostRow row{reinterpret_cast<uint8_t *>(state) + b * kCells};
            int mover = to_move[b] != 0, dn = 0, tabs = turn ? turn[b] : 0;
            uint32_t hp[2] = {hist_prev3(hist, b, 0), hist_prev3(hist, b, 1)};
            uint64_t legal = legal54(p, mover);
            for (uint32_t t = 0; t < plies; ++t) {
                const uint32_t ply = ply0 + t;
                const int pol = mover ? policy1 : policy0;
                const bool gre = pol > 0 && tabs >= opening_plies;
                GreedyResult g{-1, 0ull, false};
                int action;
                if (gre) {
                    g = greedy_decide(p, mover, legal, pol, hp[mover]);
                    action = g.fallback ? pick54(g.cands, draw32(seed, env_base + (uint64_t)b, ply, kStreamGreedy)) : g.chosen;
                    hp[mover] = (hp[mover] >> 8) | (((uint32_t)action & 0xFFu) << 16);  // :219
                } else {
                    action = sample54(legal, seed, env_base + (uint64_t)b, ply);
                }
                const Ply y = play_ply(p, row, mover, legal, action, illegal_mode);
                dn = y.terminal ? 1 : 0;
                if (y.terminal) {
                    p = Planes{0u, 0u, 0u};
                    mover = 0;
                    row.reset();
                }
                tabs = next_turn(tabs, y, 1);
                tl.games += y.terminal; tl.w1 += y.winner == 1; tl.w2 += y.winner == -1;
                legal = legal54(p, mover);
                const int64_t at = cell_of(b, t, ply_stride, tile_stride);
                if (actions_traj) actions_traj[at] = action;
                if (winner_traj) winner_traj[at] = (int8_t)y.winner;
                if (reward_traj) { reward_traj[2 * at] = (int8_t)y.r0; reward_traj[2 * at + 1] = (int8_t)y.r1; }
                if (done_traj) done_traj[at] = (int8_t)dn;
                if (to_move_traj) to_move_traj[at] = (int8_t)mover;
                if (chosen_traj) chosen_traj[at] = (gre && !g.fallback) ? g.chosen : -1;
                if (how_traj) how_traj[at] = (int8_t)(gre ? (g.fallback ? GBL_HOW_FALLBACK : GBL_HOW_GREEDY) : GBL_HOW_RANDOM);
                if (cand_traj) write_mask(cand_traj + at * kActions, gre ? g.cands : 0ull);
                if (obs_traj) write_obs(obs_traj + at * kObs, p, mover);
                if (mask_traj) write_mask(mask_traj + at * kActions, legal);
            }
            tl.plies += plies;
            to_move[b] = (int8_t)mover;
            done[b] = (int8_t)dn;
            if (turn) turn[b] = tabs;
            if (hist) {
                uint8_t *h = reinterpret_cast<uint8_t *>(hist) + b * 6;
                for (int a = 0; a < 2; ++a)
                    for (int k = 0; k < 3; ++k) h[3 * a + k] = (uint8_t)(hp[a] >> (8 * k));
            }
        }
        add_tally(counters, tl);
    });
    return GBL_OK;
}

// The boards [b0, b1) of a self-play window (c: the call, gobblet_device.h's SelfplayCall; ply0: with *ply_dev added): per ply the
// mover's search (`search(p, who, legal, g, q, S)`: false where the masked-random sampler moves, else it fills S and returns true),
// the decision or the visit-proportional draw, the step with auto-reset and the ply's cell of every trajectory array.
struct SelfplaySearch {
    HostSearch h;
    int32_t root_q;
    const uint8_t *priors;  // the root's prior row, or NULL
    // gbl_cpu_collect_search_solve's guard: the solver's V and, where it is not 0, its action -- h then holds the one-hot row and
    // the value, and nothing is decided or drawn from it; `solved`: outcome holds the solver's row
    int proven, proven_action;
    bool solved;
    int8_t outcome[kActions];
    // gbl_cpu_collect_search_tb: `judged`: tb_outcome / tb_value hold the table's verdict of the position; `table`: the mover plays from
    // it -- h holds its visits row and value, tb_action the probe's a*
    bool judged, table;
    int tb_value, tb_action;
    int8_t tb_outcome[kActions];
    // gbl_cpu_collect_search_cap: the ply is a fast one -- h holds the small search, whose visits row is not recorded
    bool fast;
    // gbl_cpu_collect_search_gumbel / gbl_cpu_collect_gumbel_solve / gbl_cpu_collect_gumbel_tb: the mover follows the Gumbel root rule -- gb holds its decision and the target row, which is recorded
    // in the visits row's place; nothing is drawn from the visits
    bool gumbel;
    HostGumbel gb;
};

extern "C++" {  // (a template cannot have the C linkage of the entry points around it)
template <typename Search>
static void selfplay_boards(int64_t b0, int64_t b1, const SelfplayCall<gbl_evaluator> &c, uint32_t ply0, Search &&search)
{
    int8_t *const state = c.state, *const to_move = c.to_move, *const done = c.done;
    const SelfplayTraj &T = c.traj;
    const int64_t ply_stride = c.ply_stride, tile_stride = c.tile_stride;
    const uint64_t seed = c.seed, env_base = c.env_base;
    const uint32_t plies = c.plies;
    const int sample_plies = c.sample_plies, illegal_mode = c.illegal_mode;
    int32_t *const turn = c.turn;
    Tally tl;
    SelfplaySearch S{};
    HostSearch &h = S.h;
    for (int64_t b = b0; b < b1; ++b) {
        uint32_t r[7];
        load_row(state, b, r);
        Planes p = make_planes(r);
        const HostRow row{reinterpret_cast<uint8_t *>(state) + b * kCells};
        const uint64_t g = env_base + (uint64_t)b;
        int mover = to_move[b] != 0, dn = 0, tabs = turn ? turn[b] : 0;
        uint64_t legal = legal54(p, mover);
        for (uint32_t t = 0; t < plies; ++t) {
            const uint32_t q = ply0 + t;
            const int who = mover;
            S.root_q = 0;
            S.priors = nullptr;
            S.proven = 0;
            S.solved = false;
            S.judged = S.table = false;
            S.fast = false;
            S.gumbel = false;
            const bool tree = search(p, who, legal, g, q, S);
            int action, how = GBL_HOW_RANDOM, value = 0;
            if (tree) {
                const bool sampled = !S.proven && !S.gumbel && tabs < sample_plies;
                action = S.proven ? S.proven_action
                         : S.gumbel ? S.gb.action
                         : sampled ? visits_pick(h.visits, draw32(seed, g, q, kStreamVisit))
                                   : S.table ? S.tb_action : tree_action_of(h.best);
                how = S.proven ? GBL_HOW_PROVEN
                      : S.gumbel ? GBL_HOW_GUMBEL
                      : S.table ? (sampled ? GBL_HOW_TABLE_SAMPLED : GBL_HOW_TABLE)
                      : S.fast  ? (sampled ? GBL_HOW_FAST_SAMPLED : GBL_HOW_FAST)
                                : sampled ? GBL_HOW_SEARCH_SAMPLED : GBL_HOW_SEARCH;
                for (int a = 0; a < kActions; ++a) value += h.wins[a] - h.losses[a];
            } else {
                action = sample54(legal, seed, g, q);
            }
            const Ply y = play_ply(p, row, mover, legal, action, illegal_mode);
            dn = y.terminal ? 1 : 0;
            if (y.terminal) {
                p = Planes{0u, 0u, 0u};
                mover = 0;
                row.reset();
            }
            tabs = next_turn(tabs, y, 1);
            tl.games += y.terminal; tl.w1 += y.winner == 1; tl.w2 += y.winner == -1;
            legal = next_mask(p, mover, dn, 1);
            const int64_t at = cell_of(b, t, ply_stride, tile_stride);
            if (T.actions) T.actions[at] = action;
            if (T.winner) T.winner[at] = (int8_t)y.winner;
            if (T.reward) { T.reward[2 * at] = (int8_t)y.r0; T.reward[2 * at + 1] = (int8_t)y.r1; }
            if (T.done) T.done[at] = (int8_t)dn;
            if (T.to_move) T.to_move[at] = (int8_t)mover;
            if (T.visits)
                for (int a = 0; a < kActions; ++a)
                    T.visits[at * kActions + a] = (int16_t)(S.gumbel ? S.gb.target[a] : tree && !S.fast ? h.visits[a] : 0);
            if (T.value) T.value[at] = value;
            if (T.nodes) T.nodes[at] = tree ? (int32_t)h.count : 0;
            if (T.how) T.how[at] = (int8_t)how;
            if (T.mover) T.mover[at] = (int8_t)who;
            if (T.root_value) T.root_value[at] = S.root_q;
            if (T.priors) {
                if (S.priors) memcpy(T.priors + at * kActions, S.priors, kActions);
                else memset(T.priors + at * kActions, 0, kActions);
            }
            if (T.outcome) {
                if (S.solved) memcpy(T.outcome + at * kActions, S.outcome, kActions);
                else memset(T.outcome + at * kActions, kSolveNone, kActions);
            }
            if (T.proven) T.proven[at] = (int8_t)S.proven;
            if (T.tb_outcome) {
                if (S.judged) memcpy(T.tb_outcome + at * kActions, S.tb_outcome, kActions);
                else memset(T.tb_outcome + at * kActions, kSolveNone, kActions);
            }
            if (T.tb_value) T.tb_value[at] = (int8_t)(S.judged ? S.tb_value : 0);
            if (T.tb_played) T.tb_played[at] = S.judged && action >= 0 ? S.tb_outcome[action] : (int8_t)kSolveNone;
            if (T.obs) write_obs(T.obs + at * kObs, p, mover);
            if (T.mask) write_mask(T.mask + at * kActions, legal);
        }
        tl.plies += plies;
        to_move[b] = (int8_t)mover;
        done[b] = (int8_t)dn;
        if (turn) turn[b] = tabs;
    }
    add_tally(c.counters, tl);
}
}  // extern "C++"

// The self-play entry points (gbl_collect_search and its _eval, _solve, _noise, _cap, _gumbel and _tb, gbl_collect_gumbel_solve and gbl_collect_gumbel_tb) behind the C ABI: the checks both flavours share (selfplay_prologue), the strides, then the boards
// over the threads.  gbl_cpu_collect_search_eval is the guarded loop with depths and weights 0 and no outcome / proven arrays;
// gbl_cpu_collect_search_tb is it with the probe in front of every ply that is judged or played from the table, and
// gbl_cpu_collect_gumbel_tb that with the Gumbel root rule on a searching side's ply (depths and weights 0).
static int host_selfplay_run(const SelfplayCall<gbl_evaluator> &c)
{
    EvalNet nets[2] = {};
    int most = 0;  // the larger tree of the sides that search
    const int go = selfplay_prologue(c, most, [](const char *why) { return fail(GBL_ERR_ARG, why); }, [&](int m) {
        if (const char *why = evaluator_pointers_error(c.ev[m])) return fail(GBL_ERR_ARG, why);
        nets[m] = eval_net(c.ev[m]);
        return GBL_OK;
    });
    if (go <= 0) return go;
    if (!strides_ok(c.n, c.plies, c.ply_stride, c.tile_stride)) return fail(GBL_ERR_ARG, kStridesMessage);
    const uint32_t ply0 = c.ply0 + (c.ply_dev ? *c.ply_dev : 0u);
    const bool uct = c.run == kRunSearch;
    const EvalNet net0 = nets[0], net1 = nets[1];
    const bool reads_table = selfplay_reads_table(c);
    const bool judge = reads_table && (c.traj.tb_outcome || c.traj.tb_value || c.traj.tb_played);
    const TbAux A = reads_table ? tb_aux(c.aux) : TbAux{};
    const TbShape tbs = reads_table ? tb_shape(c.inventory) : TbShape{};
    parallel_for(c.n, [=](int64_t b0, int64_t b1) {  // (a ply of a board is a solve and a whole search: every board is worth a thread)
        std::vector<TreeNode> nodes((size_t)most + 1);
        std::vector<uint8_t> pri(uct ? 0 : ((size_t)most + 1) * kEvalOutputs);
        uint8_t root_pi[kActions];
        selfplay_boards(b0, b1, c, ply0, [&](const Planes &p, int who, uint64_t legal, uint64_t g, uint32_t q, SelfplaySearch &S) {
            const bool plays_table = c.policy[who] == GBL_POLICY_TABLEBASE;  // (kRunTb alone admits the policy)
            if (judge || plays_table) {  // the verdict: gbl_tb_probe(mask = NULL) of the position, as its mover sees it
                const uint64_t cand = tb_board_index(A, tbs, p, who) < 0 ? 0ull : legal & tb_piece_actions(tbs);
                uint32_t best = 0;
                memset(S.tb_outcome, kSolveNone, kActions);
                for (uint32_t a = 0; a < (uint32_t)kActions; ++a)
                    if ((cand >> a) & 1ull) {
                        S.tb_outcome[a] = (int8_t)tb_probe_action(A, tbs, c.table, p, who, a);
                        best = std::max(best, tb_action_key(S.tb_outcome[a], a));
                    }
                S.judged = true;
                S.tb_value = tb_value_of(best);
                S.tb_action = tb_action_of(best);
                if (plays_table && best) {  // count on every action of O; nothing is searched
                    S.table = true;
                    S.h = HostSearch{};
                    for (uint32_t a = 0; a < (uint32_t)kActions; ++a)
                        if (((cand >> a) & 1ull) && tb_target_keeps(S.tb_outcome[a], S.tb_value, c.tb_mode)) {
                            S.h.visits[a] = c.tb_count;
                            (S.tb_value > 0 ? S.h.wins : S.h.losses)[a] = S.tb_value ? 128 * c.tb_count : 0;
                        }
                    return true;
                }
            }
            if (c.policy[who] != (uct ? GBL_POLICY_TREE : GBL_POLICY_EVAL_TREE)) return false;
            const uint32_t its = (uint32_t)c.iterations[who];
            if (uct) {
                host_tree_search(nodes, p, who, legal, g, its, (uint32_t)c.playouts[who], (uint32_t)c.max_plies, (uint32_t)c.explore, c.seed, q,
                                 S.h);
                return true;
            }
            uint64_t cand = legal;
            if (c.solve_depth[who] > 0 && legal) {
                const uint32_t best = host_solve(p, who, legal, c.solve_depth[who], S.outcome);
                S.solved = true;
                S.proven = solve_value_of(best);
                if (S.proven) {  // the one-hot row and the value of a proven root: no search
                    S.proven_action = solve_action_of(best);
                    S.h = HostSearch{};
                    S.h.visits[S.proven_action] = (int)its;
                    (S.proven > 0 ? S.h.wins : S.h.losses)[S.proven_action] = 128 * (int)its;
                    return true;
                }
                cand = 0;
                for (int a = 0; a < kActions; ++a) cand |= (uint64_t)(S.outcome[a] == 0) << a;
            }
            // (the playout cap's draw, after the guard: a proven ply takes none)
            const CapPly cp = cap_ply(c.seed, g, q, (uint32_t)selfplay_share(c, who), its, (uint32_t)c.fast[who], (uint32_t)c.noise[who]);
            S.fast = cp.fast;
            S.gumbel = selfplay_considered(c, who) != 0;
            S.gb = HostGumbel{GumbelArgs{(uint32_t)selfplay_considered(c, who), (uint32_t)c.gumbel_noise, (uint32_t)c.visit_offset, (uint32_t)c.scale},
                              c.seed, g, q, -1, {}, {}};
            S.root_q = host_tree_search_eval(nodes, pri, who ? net1 : net0, p, who, cand, cp.its, (uint32_t)c.explore, S.h,
                                             HostNoise{cp.noise, c.seed, g, q, root_pi}, S.gumbel ? &S.gb : nullptr);
            S.priors = root_pi;  // (the network's row; zeros where the root has no candidate)
            return true;
        });
    }, 1);
    return GBL_OK;
}

// the nine entry points themselves: one text for both flavours (the host flavour's calls are synchronous: `stream` is not read)
#define GBL_SYMBOL(fn) gbl_cpu_##fn
#define GBL_SELFPLAY_RUN(name, call, stream) ((void)(stream), host_selfplay_run(call))
#include "gobblet_selfplay_entries.inc"
#include "gobblet_env_entries.inc"  // (gbl_cpu_step, _step_into, _sample, _rollout, _collect, _collect_from, _greedy_act: they only forward)
#undef GBL_SYMBOL
#undef GBL_SELFPLAY_RUN

int gbl_cpu_outcome_targets(const int8_t *done_traj, const int8_t *reward_traj, const int8_t *mover_traj, int8_t *z_traj,
                            int16_t *plies_left_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint32_t plies, void *)
{
    if (const char *why = outcome_targets_error(n, done_traj, reward_traj, mover_traj, z_traj, plies, ply_stride, tile_stride))
        return fail(GBL_ERR_ARG, why);
    if (n == 0 || plies == 0) return GBL_OK;
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) {
            int r0 = 0, r1 = 0, left = -1;  // the rewards of the nearest game end at or after t, and how far it is
            for (uint32_t t = plies; t-- > 0;) {
                const int64_t at = cell_of(b, t, ply_stride, tile_stride);
                if (done_traj[at]) { r0 = reward_traj[2 * at]; r1 = reward_traj[2 * at + 1]; left = 0; }
                else if (left >= 0) ++left;
                z_traj[at] = (int8_t)(left < 0 ? GBL_Z_OPEN : (mover_traj[at] ? r1 : r0));
                if (plies_left_traj) plies_left_traj[at] = (int16_t)left;
            }
        }
    });
    return GBL_OK;
}

int gbl_cpu_symmetry_apply(const int16_t *sym, int sym_all, const int8_t *agent, const int8_t *state_in, int8_t *state_out,
                           const int8_t *obs_in, int8_t *obs_out, const int8_t *mask_in, int8_t *mask_out, const int16_t *visits_in,
                           int16_t *visits_out, const uint8_t *priors_in, uint8_t *priors_out, const int32_t *actions_in,
                           int32_t *actions_out, int64_t n, void *)
{
    const SymRowsArg R{{state_in, obs_in, mask_in, visits_in, priors_in, actions_in},
                       {state_out, obs_out, mask_out, visits_out, priors_out, actions_out}};
    if (const char *why = symmetry_error(sym, sym_all, agent, R, n)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) {
            const Sym S = sym_of((uint32_t)(sym ? sym[b] : sym_all) & 511u);
            const uint32_t m = agent && agent[b] != 0;
            if (state_in) sym_state_row(state_in + b * kCells, state_out + b * kCells, S);
            if (obs_in) sym_obs_row(obs_in + b * kObs, obs_out + b * kObs, S, m);
            if (mask_in) sym_action_row(mask_in + b * kActions, mask_out + b * kActions, S, m);
            if (visits_in) sym_action_row(visits_in + b * kActions, visits_out + b * kActions, S, m);
            if (priors_in) sym_action_row(priors_in + b * kActions, priors_out + b * kActions, S, m);
            if (actions_in) actions_out[b] = sym_action_any(S, m, actions_in[b]);
        }
    });
    return GBL_OK;
}

int gbl_cpu_training_batch(const int8_t *obs_traj, const int8_t *mask_traj, const int16_t *visits_traj, const int8_t *z_traj,
                           const int8_t *done_traj, const int8_t *mover_traj, int64_t n, uint32_t plies, int64_t ply_stride,
                           int64_t tile_stride, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base, uint32_t call,
                           int8_t *obs_out, int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out, int16_t *sym_out,
                           void *)
{
    if (const char *why = batch_error(obs_traj, mask_traj, visits_traj, z_traj, done_traj, mover_traj, n, plies, ply_stride, tile_stride,
                                      batch, sym_mask, call, obs_out, mask_out, index_out))
        return fail(GBL_ERR_ARG, why);
    if (batch == 0) return GBL_OK;
    parallel_for(batch, [=](int64_t j0, int64_t j1) {
        for (int64_t j = j0; j < j1; ++j) {
            int64_t at = -1, prev = -1;
            BatchDraw d{0u, 0u, 0};
            for (uint32_t i = 0; i < (uint32_t)kBatchAttempts && at < 0; ++i) {
                d = batch_draw(seed, sample_base + (uint64_t)j, call, i, plies, n);
                const int64_t c = traj_cell(d.t, d.b, ply_stride, tile_stride), p = traj_cell((int64_t)d.t - 1, d.b, ply_stride, tile_stride);
                if (batch_valid(z_traj, done_traj, visits_traj, c, p)) { at = c; prev = p; }
            }
            const bool ok = at >= 0;
            const uint32_t code = ok ? d.sym & (uint32_t)sym_mask : 0u;
            index_out[2 * j] = ok ? (int32_t)d.t : -1;
            index_out[2 * j + 1] = ok ? (int32_t)d.b : -1;
            if (z_out) z_out[j] = ok ? z_traj[at] : (int8_t)kZOpen;
            if (sym_out) sym_out[j] = (int16_t)code;
            if (!ok) {
                if (obs_out) memset(obs_out + j * kObs, 0, kObs);
                if (mask_out) memset(mask_out + j * kActions, 0, kActions);
                if (visits_out) memset(visits_out + j * kActions, 0, 2 * kActions);
                continue;
            }
            const Sym S = sym_of(code);
            const uint32_t m = mover_traj[at] != 0;
            if (obs_out) sym_obs_row(obs_traj + prev * kObs, obs_out + j * kObs, S, m);
            if (mask_out) sym_action_row(mask_traj + prev * kActions, mask_out + j * kActions, S, m);
            if (visits_out) sym_action_row(visits_traj + at * kActions, visits_out + j * kActions, S, m);
        }
    });
    return GBL_OK;
}

// The header's enumeration as it reads: the cells in ascending (t, b), counted once and then walked again with their ranks (one
// thread: the order is the rule).  The workspace is checked like the device flavour's and not used.
int gbl_cpu_replay_append(const int8_t *obs_traj, const int8_t *mask_traj, const int16_t *visits_traj, const int8_t *z_traj,
                          const int8_t *done_traj, const int8_t *mover_traj, int64_t n, uint32_t plies, int64_t ply_stride,
                          int64_t tile_stride, int32_t tag, int8_t *ring_obs, int16_t *ring_visits, int8_t *ring_meta, int64_t capacity,
                          uint64_t *ring_state, void *workspace, size_t workspace_bytes, void *)
{
    if (const char *why = replay_append_error(obs_traj, mask_traj, visits_traj, z_traj, done_traj, mover_traj, n, plies, ply_stride,
                                              tile_stride, ring_obs, ring_visits, ring_meta, capacity, ring_state, workspace, workspace_bytes))
        return fail(GBL_ERR_ARG, why);
    const auto valid = [=](uint32_t t, int64_t b) {
        return batch_valid(z_traj, done_traj, visits_traj, traj_cell(t, b, ply_stride, tile_stride), traj_cell((int64_t)t - 1, b, ply_stride, tile_stride));
    };
    uint64_t K = 0, R = 0;
    for (uint32_t t = 1; t < plies; ++t)
        for (int64_t b = 0; b < n; ++b) K += valid(t, b);
    const uint64_t T0 = ring_state[0], cap = (uint64_t)capacity;
    for (uint32_t t = 1; t < plies; ++t) {
        for (int64_t b = 0; b < n; ++b) {
            if (!valid(t, b)) continue;
            const uint64_t r = R++;
            if (!replay_kept(r, K, cap)) continue;
            const int64_t slot = replay_slot(T0, r, cap), at = traj_cell(t, b, ply_stride, tile_stride),
                          prev = traj_cell((int64_t)t - 1, b, ply_stride, tile_stride);
            if (ring_obs) {
                int8_t *o = ring_obs + slot * kReplayObsPitch;
                memcpy(o, obs_traj + prev * kObs, kObs);
                memset(o + kObs, 0, kReplayObsPitch - kObs);
            }
            int16_t *v = ring_visits + slot * kReplayVisitsPitch;
            memcpy(v, visits_traj + at * kActions, 2 * kActions);
            memset(v + kActions, 0, 2 * (kReplayVisitsPitch - kActions));
            int8_t *m = ring_meta + slot * kReplayMetaPitch;
            memcpy(m, mask_traj + prev * kActions, kActions);
            m[kReplayMetaZ] = z_traj[at];
            m[kReplayMetaMover] = (int8_t)(mover_traj[at] != 0);
            for (int i = 0; i < 4; ++i) m[kReplayMetaTag + i] = (int8_t)((uint32_t)tag >> (8 * i));
            memset(m + kReplayMetaTag + 4, 0, kReplayMetaPitch - kReplayMetaTag - 4);
        }
    }
    ring_state[0] = T0 + K;
    ring_state[1] = K;
    return GBL_OK;
}

int gbl_cpu_replay_batch(const int8_t *ring_obs, const int16_t *ring_visits, const int8_t *ring_meta, int64_t capacity,
                         const uint64_t *ring_state, int64_t recent, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base,
                         uint32_t call, int8_t *obs_out, int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out,
                         int16_t *sym_out, void *)
{
    if (const char *why = replay_batch_error(ring_obs, ring_visits, ring_meta, capacity, ring_state, recent, batch, sym_mask, call, obs_out,
                                             index_out))
        return fail(GBL_ERR_ARG, why);
    if (batch == 0) return GBL_OK;
    const uint64_t total = ring_state[0];
    parallel_for(batch, [=](int64_t j0, int64_t j1) {
        for (int64_t j = j0; j < j1; ++j) {
            const ReplayDraw d = replay_draw(seed, sample_base + (uint64_t)j, call, total, (uint64_t)capacity, recent);
            const bool ok = d.slot >= 0;
            const uint32_t code = ok ? d.sym & (uint32_t)sym_mask : 0u;
            const int8_t *meta = ring_meta + (ok ? d.slot : 0) * kReplayMetaPitch;
            int32_t tag = -1;
            if (ok) memcpy(&tag, meta + kReplayMetaTag, 4);
            index_out[2 * j] = ok ? (int32_t)d.slot : -1;
            index_out[2 * j + 1] = tag;
            if (z_out) z_out[j] = ok ? meta[kReplayMetaZ] : (int8_t)kZOpen;
            if (sym_out) sym_out[j] = (int16_t)code;
            if (!ok) {
                if (obs_out) memset(obs_out + j * kObs, 0, kObs);
                if (mask_out) memset(mask_out + j * kActions, 0, kActions);
                if (visits_out) memset(visits_out + j * kActions, 0, 2 * kActions);
                continue;
            }
            const Sym S = sym_of(code);
            const uint32_t m = meta[kReplayMetaMover] != 0;
            if (obs_out) sym_obs_row(ring_obs + d.slot * kReplayObsPitch, obs_out + j * kObs, S, m);
            if (mask_out) sym_action_row(meta, mask_out + j * kActions, S, m);
            if (visits_out) sym_action_row(ring_visits + d.slot * kReplayVisitsPitch, visits_out + j * kActions, S, m);
        }
    });
    return GBL_OK;
}

// Prioritised replay as the header's paragraph reads.  The append's cells are enumerated again (the workspace is checked and not used);
// the index has the device flavour's layout, built by one walk over the slots; a draw is replay_prio_span and replay_prio_draw, the pieces
// the kernel uses.
int gbl_cpu_replay_prio_append(const int16_t *visits_traj, const int8_t *z_traj, const int8_t *done_traj, const int32_t *prio_traj, int32_t value,
                               int64_t n, uint32_t plies, int64_t ply_stride, int64_t tile_stride, int32_t *ring_prio, int64_t capacity,
                               const uint64_t *ring_state, const void *workspace, size_t workspace_bytes, void *)
{
    if (const char *why = replay_prio_append_error(visits_traj, z_traj, done_traj, n, plies, ply_stride, tile_stride, ring_prio, capacity,
                                                   ring_state, workspace, workspace_bytes))
        return fail(GBL_ERR_ARG, why);
    const uint64_t K = ring_state[1], T0 = ring_state[0] - K, cap = (uint64_t)capacity;
    uint64_t R = 0;
    for (uint32_t t = 1; t < plies; ++t) {
        for (int64_t b = 0; b < n; ++b) {
            const int64_t at = traj_cell(t, b, ply_stride, tile_stride);
            if (!batch_valid(z_traj, done_traj, visits_traj, at, traj_cell((int64_t)t - 1, b, ply_stride, tile_stride))) continue;
            const uint64_t r = R++;
            if (replay_kept(r, K, cap)) ring_prio[replay_slot(T0, r, cap)] = prio_traj ? prio_traj[at] : value;
        }
    }
    return GBL_OK;
}

int gbl_cpu_replay_prio_update(const int32_t *index, const int32_t *values, int64_t batch, int32_t *ring_prio, int64_t capacity, void *)
{
    if (const char *why = replay_prio_update_error(index, values, batch, ring_prio, capacity)) return fail(GBL_ERR_ARG, why);
    const auto named = [=](int64_t j) { return index[2 * j] >= 0 && (int64_t)index[2 * j] < capacity; };
    for (int64_t j = 0; j < batch; ++j)
        if (named(j)) ring_prio[index[2 * j]] = INT32_MIN;
    for (int64_t j = 0; j < batch; ++j)
        if (named(j)) ring_prio[index[2 * j]] = std::max(ring_prio[index[2 * j]], values[j]);
    return GBL_OK;
}

int gbl_cpu_replay_prio_index(const int32_t *ring_prio, int64_t capacity, const uint64_t *ring_state, void *prio_index, size_t index_bytes, void *)
{
    if (const char *why = replay_prio_index_error(ring_prio, capacity, ring_state, prio_index, index_bytes)) return fail(GBL_ERR_ARG, why);
    uint64_t *index = static_cast<uint64_t *>(prio_index);
    const uint64_t total = ring_state[0], cap = (uint64_t)capacity, live = std::min(total, cap);
    const uint64_t leaves = replay_prio_leaves(cap), blocks = replay_prio_blocks(cap);
    uint64_t *base = index + kReplayPrioHead, *local = base + blocks + 1u;
    uint64_t acc = 0, in_block = 0;
    for (uint64_t L = 0; L < leaves; ++L) {
        if (L % kReplayBlockLeaves == 0) {
            base[L / kReplayBlockLeaves] = acc;
            in_block = 0;
        }
        local[L] = in_block;
        uint64_t leaf = 0;
        for (uint64_t s = L * kReplayLeaf; s < std::min((L + 1) * kReplayLeaf, live); ++s) leaf += replay_weight(ring_prio[s]);
        acc += leaf;
        in_block += leaf;
    }
    base[blocks] = acc;
    index[0] = total;
    index[1] = acc;
    return GBL_OK;
}

int gbl_cpu_replay_batch_prio(const int8_t *ring_obs, const int16_t *ring_visits, const int8_t *ring_meta, int64_t capacity,
                              const uint64_t *ring_state, const int32_t *ring_prio, const void *prio_index, int32_t *prio_out,
                              uint64_t *total_out, int64_t recent, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base,
                              uint32_t call, int8_t *obs_out, int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out,
                              int16_t *sym_out, void *)
{
    if (const char *why = replay_batch_prio_error(ring_obs, ring_visits, ring_meta, capacity, ring_state, ring_prio, prio_index, recent, batch,
                                                  sym_mask, call, obs_out, index_out))
        return fail(GBL_ERR_ARG, why);
    if (batch == 0) return GBL_OK;
    const uint64_t *index = static_cast<const uint64_t *>(prio_index);
    const ReplayPrioSpan P = replay_prio_span(ring_prio, index, ring_state[0], (uint64_t)capacity, recent);
    if (total_out) { total_out[0] = P.W; total_out[1] = P.span; }
    parallel_for(batch, [=](int64_t j0, int64_t j1) {
        for (int64_t j = j0; j < j1; ++j) {
            const ReplayPrioDraw d = replay_prio_draw(seed, sample_base + (uint64_t)j, call, P, (uint64_t)capacity, ring_prio, index);
            const bool ok = d.slot >= 0;
            const uint32_t code = ok ? d.sym & (uint32_t)sym_mask : 0u;
            const int8_t *meta = ring_meta + (ok ? d.slot : 0) * kReplayMetaPitch;
            int32_t tag = -1;
            if (ok) memcpy(&tag, meta + kReplayMetaTag, 4);
            index_out[2 * j] = ok ? (int32_t)d.slot : -1;
            index_out[2 * j + 1] = tag;
            if (prio_out) prio_out[j] = (int32_t)d.weight;
            if (z_out) z_out[j] = ok ? meta[kReplayMetaZ] : (int8_t)kZOpen;
            if (sym_out) sym_out[j] = (int16_t)code;
            if (!ok) {
                if (obs_out) memset(obs_out + j * kObs, 0, kObs);
                if (mask_out) memset(mask_out + j * kActions, 0, kActions);
                if (visits_out) memset(visits_out + j * kActions, 0, 2 * kActions);
                continue;
            }
            const Sym S = sym_of(code);
            const uint32_t m = meta[kReplayMetaMover] != 0;
            if (obs_out) sym_obs_row(ring_obs + d.slot * kReplayObsPitch, obs_out + j * kObs, S, m);
            if (mask_out) sym_action_row(meta, mask_out + j * kActions, S, m);
            if (visits_out) sym_action_row(ring_visits + d.slot * kReplayVisitsPitch, visits_out + j * kActions, S, m);
        }
    });
    return GBL_OK;
}

// The tablebase (include/gobblet_hip.h, "Exact tablebase"): the header's rule position by position, with the shared pieces of
// gobblet_device.h.  aux, table and decided are host memory.
int gbl_cpu_tb_prepare(const int32_t *inventory, void *aux, void *)
{
    if (const char *why = tb_inventory_error(inventory)) return fail(GBL_ERR_ARG, why);
    if (!aux) return fail(GBL_ERR_ARG, "aux must not be NULL");
    uint8_t *b = static_cast<uint8_t *>(aux);
    memset(b, 0, kTbAuxBytes);
    uint16_t *rank2 = reinterpret_cast<uint16_t *>(b + kTbAuxRank2), *inv2 = reinterpret_cast<uint16_t *>(b + kTbAuxInv2),
             *inv1 = reinterpret_cast<uint16_t *>(b + kTbAuxInv1), *tern = reinterpret_cast<uint16_t *>(b + kTbAuxTern);
    uint8_t *rank1 = b + kTbAuxRank1;
    uint32_t n2 = 0, n1 = 0;
    for (uint32_t t = 0; t < kTbTernary; ++t) {
        const uint32_t f = tb_admissible(t);
        rank2[t] = (f & 1u) ? (uint16_t)n2 : (uint16_t)0xFFFFu;
        rank1[t] = (f >> 16) ? (uint8_t)n1 : (uint8_t)0xFFu;
        if (f & 1u) inv2[n2++] = (uint16_t)t;
        if (f >> 16) inv1[n1++] = (uint16_t)t;
    }
    for (uint32_t cells = 0; cells < 512u; ++cells) tern[cells] = (uint16_t)tb_tern_of(cells);
    return GBL_OK;
}

int gbl_cpu_tb_sweep(const int32_t *inventory, const void *aux, const int8_t *table, int8_t *out, int64_t first, int64_t count, int k,
                     uint64_t *decided, void *)
{
    if (const char *why = tb_sweep_error(inventory, aux, table, out, first, count, k, decided)) return fail(GBL_ERR_ARG, why);
    if (count == 0) return GBL_OK;
    const TbAux A = tb_aux(aux);
    const TbShape S = tb_shape(inventory);
    std::atomic<uint64_t> wrote{0};
    std::atomic<uint64_t> *const total = &wrote;
    parallel_for(count, [=](int64_t j0, int64_t j1) {
        uint64_t mine = 0;
        for (int64_t j = j0; j < j1; ++j) {
            if (k > 0 && out[j] != 0) continue;
            const TbPos p = tb_position_of(A, S, (uint32_t)(first + j));
            const int v = k == 0 ? (tb_winner(p.own, p.oth) != 0 ? kTbTerminal : 0) : tb_sweep_value(A, S, p, k, table);
            if (k == 0) out[j] = (int8_t)v;
            else if (v == k || v == -k) out[j] = (int8_t)v;
            else continue;
            mine += v != 0;
        }
        total->fetch_add(mine);
    });
    *decided += wrote.load();
    return GBL_OK;
}

int gbl_cpu_tb_index(const int32_t *inventory, const void *aux, const int8_t *state, const int8_t *to_move, int64_t *index_out, int64_t n,
                     void *)
{
    if (const char *why = tb_rows_error(inventory, aux, n, state, "state must not be NULL", to_move, "to_move must not be NULL", index_out,
                                        "index_out must not be NULL"))
        return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    const TbAux A = tb_aux(aux);
    const TbShape S = tb_shape(inventory);
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) {
            uint32_t r[7];
            load_row(state, b, r);
            index_out[b] = tb_board_index(A, S, make_planes(r), to_move[b] != 0);
        }
    });
    return GBL_OK;
}

int gbl_cpu_tb_position(const int32_t *inventory, const void *aux, const int64_t *index, int8_t *state_out, int64_t n, void *)
{
    if (const char *why = tb_rows_error(inventory, aux, n, index, "index must not be NULL", state_out, "state_out must not be NULL", state_out, ""))
        return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    const TbAux A = tb_aux(aux);
    const TbShape S = tb_shape(inventory);
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) tb_row_of(A, S, index[b], state_out + b * kCells);
    });
    return GBL_OK;
}

int gbl_cpu_tb_probe(const int32_t *inventory, const void *aux, const int8_t *table, const int8_t *state, const int8_t *to_move,
                     const int8_t *mask, int8_t *outcome_out, int8_t *value_out, int32_t *action_out, int64_t n, void *)
{
    if (const char *why = tb_rows_error(inventory, aux, n, table, "table must not be NULL", state, "state must not be NULL", to_move,
                                        "to_move must not be NULL"))
        return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    if (reinterpret_cast<uintptr_t>(action_out) & 3u) return fail(GBL_ERR_ALIGN, "action_out must be 4-byte aligned");
    const TbAux A = tb_aux(aux);
    const TbShape S = tb_shape(inventory);
    parallel_for(n, [=](int64_t b0, int64_t b1) {
        for (int64_t b = b0; b < b1; ++b) {
            const HostRoot R = host_root(state, to_move, mask, b);
            const uint64_t cand = tb_board_index(A, S, R.p, R.mover) < 0 ? 0ull : R.cand & tb_piece_actions(S);
            uint32_t best = 0;
            for (uint32_t a = 0; a < (uint32_t)kActions; ++a) {
                int c = kSolveNone;
                if ((cand >> a) & 1ull) {
                    c = tb_probe_action(A, S, table, R.p, R.mover, a);
                    best = std::max(best, tb_action_key(c, a));
                }
                if (outcome_out) outcome_out[b * kActions + a] = (int8_t)c;
            }
            if (value_out) value_out[b] = (int8_t)tb_value_of(best);
            if (action_out) action_out[b] = tb_action_of(best);
        }
    });
    return GBL_OK;
}

// Tablebase targets (include/gobblet_hip.h, "Tablebase targets"): decode_obs_row, the probe's loop and the rule's scalar pieces, row by
// row.  The visits rows go through memcpy: the host flavour asks no alignment of them.
int gbl_cpu_tb_targets(const int32_t *inventory, const void *aux, const int8_t *table, const int8_t *obs, int64_t obs_pitch, const int8_t *mask,
                       int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch, const int8_t *z_in,
                       int8_t *z_out, int64_t z_pitch, int mode, int count, int8_t *value_out, int8_t *outcome_out, int8_t *census_out,
                       int64_t n, void *)
{
    bool empty;
    if (const char *why = tb_targets_error(inventory, aux, table, obs, obs_pitch, mask, mask_pitch, visits_in, visits_out, visits_pitch, z_in,
                                           z_out, z_pitch, mode, count, value_out, outcome_out, census_out, n, &empty))
        return fail(GBL_ERR_ARG, why);
    if (empty) return GBL_OK;
    const TbAux A = tb_aux(aux);
    const TbShape S = tb_shape(inventory);
    const char *vin = reinterpret_cast<const char *>(visits_in);
    char *vout = reinterpret_cast<char *>(visits_out);
    parallel_for(n, [=](int64_t r0, int64_t r1) {
        for (int64_t r = r0; r < r1; ++r) {
            const int z_old = z_in ? (int)z_in[r * z_pitch] : 0;
            int8_t c[kActions];
            memset(c, kSolveNone, sizeof c);
            int value = 0, census = -1;
            const bool skipped = z_in && z_old == kZOpen;
            if (!skipped) {
                uint32_t d[30], row[7];
                d[29] = 0;
                memcpy(d, obs + r * obs_pitch, kObs);
                const int mover = decode_obs_row(d, row) != 0;
                const Planes p = make_planes(row);
                uint64_t cand = legal54(p, mover) & tb_piece_actions(S);
                if (mask) cand &= read_mask(mask + r * mask_pitch);
                if (tb_board_index(A, S, p, mover) < 0) cand = 0;
                uint32_t best = 0;
                for (uint32_t a = 0; a < (uint32_t)kActions; ++a)
                    if ((cand >> a) & 1ull) {
                        c[a] = (int8_t)tb_probe_action(A, S, table, p, mover, a);
                        best = std::max(best, tb_action_key(c[a], a));
                    }
                value = tb_value_of(best);
                int16_t old[kActions], now[kActions];
                if (visits_in) memcpy(old, vin + r * visits_pitch * 2, sizeof old);  // (read before the row is written: it may be the same row)
                uint64_t keeps = 0;
                uint32_t top = 0;
                for (uint32_t a = 0; a < (uint32_t)kActions; ++a) {
                    const bool mine = (cand >> a) & 1ull;
                    keeps |= (uint64_t)(mine && tb_target_keeps(c[a], value, kTbTargetResult)) << a;
                    now[a] = (int16_t)(best && mine && tb_target_keeps(c[a], value, mode) ? count : 0);
                    if (visits_in) top = std::max(top, tb_visit_key(old[a], a));
                }
                if (best) census = tb_census(top, keeps, z_in != nullptr, z_old, tb_sign(value));
                if (visits_out) memcpy(vout + r * visits_pitch * 2, now, sizeof now);
                z_out[r * z_pitch] = (int8_t)(best ? tb_sign(value) : kZOpen);
            }
            if (value_out) value_out[r] = (int8_t)value;
            if (outcome_out) memcpy(outcome_out + r * kActions, c, sizeof c);
            if (census_out) census_out[r] = (int8_t)census;
        }
    });
    return GBL_OK;
}

// Reanalysis (include/gobblet_hip.h, "Reanalysis"): decode_obs_row, host_tree_search_eval and the rule's scalar pieces, row by row.  The
// visits rows go through memcpy: the host flavour asks no alignment of them.  gum: gbl_cpu_reanalyse_gumbel's arguments (nullptr:
// gbl_cpu_reanalyse) -- the root follows the Gumbel rule (GumbelRoot, board id env_base + r), the row's new entries are the target bytes
// and the drift's sum is 64-bit.
static int host_reanalyse(const gbl_evaluator *ev, int iterations, int explore, const ReanalyseGumbelCheck *gum, uint64_t seed,
                          const int8_t *obs, int64_t obs_pitch, const int8_t *mask, int64_t mask_pitch, const int16_t *visits_in,
                          int16_t *visits_out, int64_t visits_pitch, const int8_t *z_in, int64_t z_pitch, int32_t *root_value_out,
                          uint8_t *root_priors_out, int32_t *action_out, int32_t *nodes_out, int32_t *drift_out, int8_t *census_out, int64_t n)
{
    bool empty;
    if (const char *why = reanalyse_error(ev, iterations, explore, obs, obs_pitch, mask, mask_pitch, visits_in, visits_out, visits_pitch, z_in,
                                          z_pitch, root_value_out, root_priors_out, action_out, nodes_out, drift_out, census_out, n, &empty, gum))
        return fail(GBL_ERR_ARG, why);
    if (empty) return GBL_OK;
    const EvalNet net = eval_net(ev);
    const char *vin = reinterpret_cast<const char *>(visits_in);
    char *vout = reinterpret_cast<char *>(visits_out);
    const bool rule = gum != nullptr;
    const ReanalyseGumbelCheck g = rule ? *gum : ReanalyseGumbelCheck{};
    char *const gout = reinterpret_cast<char *>(const_cast<void *>(g.gumbel_out));
    parallel_for(n, [=](int64_t r0, int64_t r1) {  // (a row is a whole search: every row is worth a thread)
        std::vector<TreeNode> nodes((size_t)iterations + 1);
        std::vector<uint8_t> pri(((size_t)iterations + 1) * kEvalOutputs);
        HostSearch h;
        HostGumbel gb{GumbelArgs{(uint32_t)g.considered, (uint32_t)g.gumbel_noise, (uint32_t)g.visit_offset, (uint32_t)g.scale}, seed, 0, g.call,
                      -1, {}, {}};
        for (int64_t r = r0; r < r1; ++r) {
            const int z_old = z_in ? (int)z_in[r * z_pitch] : 0;
            int q = 0, action = -1, drift = -1, census = -1, count = 0;
            uint8_t pi[kActions] = {};
            memset(gb.gum, 0, sizeof gb.gum);
            if (!(z_in && z_old == kZOpen)) {
                uint32_t d[30], row[7];
                d[29] = 0;
                memcpy(d, obs + r * obs_pitch, kObs);
                const int mover = decode_obs_row(d, row) != 0;
                const Planes p = make_planes(row);
                uint64_t cand = legal54(p, mover);
                if (mask) cand &= read_mask(mask + r * mask_pitch);
                gb.g = g.env_base + (uint64_t)r;
                q = host_tree_search_eval(nodes, pri, net, p, mover, cand, (uint32_t)iterations, (uint32_t)explore, h, HostNoise{0, 0, 0, 0, pi},
                                          rule ? &gb : nullptr);
                action = rule ? gb.action : tree_action_of(h.best);
                count = (int)h.count;
                int16_t old[kActions] = {}, now[kActions];
                if (visits_in) memcpy(old, vin + r * visits_pitch * 2, sizeof old);  // (read before the row is written: it may be the same row)
                uint32_t So = 0, Sn = 0, top_old = 0, top_new = 0;
                uint64_t diff = 0;
                for (uint32_t a = 0; a < (uint32_t)kActions; ++a) {
                    now[a] = (int16_t)(rule ? (uint32_t)gb.target[a] : h.visits[a]);
                    So += (uint32_t)std::max<int>(old[a], 0);
                    Sn += (uint32_t)now[a];
                }
                for (uint32_t a = 0; a < (uint32_t)kActions; ++a) {
                    const uint32_t x = (uint32_t)std::max<int>(old[a], 0) * Sn, y = (uint32_t)now[a] * So;
                    diff += x > y ? x - y : y - x;
                    top_old = std::max(top_old, tb_visit_key(old[a], a));
                    top_new = std::max(top_new, tb_visit_key(now[a], a));
                }
                if (cand) {
                    drift = rule ? reanalyse_drift64(visits_in != nullptr, So, Sn, diff) : reanalyse_drift(visits_in != nullptr, So, Sn, (uint32_t)diff);
                    census = reanalyse_census(top_old, top_new, z_in != nullptr, z_old, q);
                }
                if (visits_out) memcpy(vout + r * visits_pitch * 2, now, sizeof now);
            }
            if (root_value_out) root_value_out[r] = q;
            if (root_priors_out) memcpy(root_priors_out + r * kActions, pi, sizeof pi);
            if (action_out) action_out[r] = action;
            if (nodes_out) nodes_out[r] = count;
            if (drift_out) drift_out[r] = drift;
            if (census_out) census_out[r] = (int8_t)census;
            if (gout) memcpy(gout + r * kActions * 2, gb.gum, sizeof gb.gum);
        }
    }, 1);
    return GBL_OK;
}

int gbl_cpu_reanalyse(const gbl_evaluator *ev, int iterations, int explore, const int8_t *obs, int64_t obs_pitch, const int8_t *mask,
                      int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch, const int8_t *z_in,
                      int64_t z_pitch, int32_t *root_value_out, uint8_t *root_priors_out, int32_t *action_out, int32_t *nodes_out,
                      int32_t *drift_out, int8_t *census_out, int64_t n, void *)
{
    return host_reanalyse(ev, iterations, explore, nullptr, 0, obs, obs_pitch, mask, mask_pitch, visits_in, visits_out, visits_pitch, z_in, z_pitch,
                          root_value_out, root_priors_out, action_out, nodes_out, drift_out, census_out, n);
}

int gbl_cpu_reanalyse_gumbel(const gbl_evaluator *ev, int iterations, int explore, int considered, int gumbel_noise, int visit_offset,
                             int scale, uint64_t seed, uint64_t env_base, uint32_t call, const int8_t *obs, int64_t obs_pitch,
                             const int8_t *mask, int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch,
                             const int8_t *z_in, int64_t z_pitch, int32_t *root_value_out, uint8_t *root_priors_out, int32_t *action_out,
                             int32_t *nodes_out, int32_t *drift_out, int8_t *census_out, int16_t *gumbel_out, int64_t n, void *)
{
    const ReanalyseGumbelCheck check{considered, gumbel_noise, visit_offset, scale, env_base, call, gumbel_out};
    return host_reanalyse(ev, iterations, explore, &check, seed, obs, obs_pitch, mask, mask_pitch, visits_in, visits_out, visits_pitch, z_in,
                          z_pitch, root_value_out, root_priors_out, action_out, nodes_out, drift_out, census_out, n);
}

}  // extern "C"

// gbl_cpu_train_step: the header's rule row by row and element by element -- the same scalar pieces (gobblet_device.h: train_exp,
// train_log, train_value, train_policy, train_gradient, train_adam) in the same order as the kernels; the rows, and then the
// parameter segments, are dealt over the threads, which changes no sum's order.
namespace {

struct HostTrain {
    const int8_t *obs, *mask;
    const int16_t *visits;
    const int8_t *z;
    const float *params;
    float *h, *dh, *dout, *row;
    int H;
    TrainHyper hy;
    // gbl_cpu_train_step_weighted alone (EX): the rows' weights and the two per-row outputs
    const float *row_weight;
    float *row_loss_out;
    int32_t *prio_out;
    float prio_scale;
    int32_t prio_floor, prio_cap;
};

template <bool EX>
void train_row(const HostTrain &A, int64_t r)
{
    GBL_FP_STRICT
    const int H = A.H;
    float *rh = A.h + r * H, *rdh = A.dh + r * H, *rdo = A.dout + r * kTrainDoStride, *rst = A.row + r * kTrainRowStats;
    const float *w1 = A.params, *b1 = w1 + kObs * H, *w2 = b1 + H, *b2 = w2 + H * kTrainOutputs;
    bool in_c[kActions];
    int S = 0, first = -1;
    for (int a = 0; a < kActions; ++a) {
        in_c[a] = !A.mask || A.mask[r * kActions + a] != 0;
        if (in_c[a]) S += A.visits[r * kActions + a];
        if (in_c[a] && first < 0) first = a;
    }
    const int z = A.z[r];
    if (z == kZOpen || S <= 0) {
        std::fill(rh, rh + H, 0.0f); std::fill(rdh, rdh + H, 0.0f);
        std::fill(rdo, rdo + kTrainDoStride, 0.0f); std::fill(rst, rst + kTrainRowStats, 0.0f);
        if (EX && A.row_loss_out) A.row_loss_out[2 * r] = A.row_loss_out[2 * r + 1] = 0.0f;
        if (EX && A.prio_out) A.prio_out[r] = 0;
        return;
    }
    float pre[256], o[kTrainOutputs], d[kActions], e[kActions], term[kActions];
    for (int j = 0; j < H; ++j) pre[j] = b1[j];
    for (int f = 0; f < kObs; ++f)
        if (A.obs[r * kObs + f] != 0)
            for (int j = 0; j < H; ++j) pre[j] = pre[j] + w1[f * H + j];
    float top = 0.0f;
    for (int j = 0; j < H; ++j) {
        rh[j] = pre[j] > 0.0f ? pre[j] : 0.0f;
        top = train_float_bits(rh[j]) > train_float_bits(top) ? rh[j] : top;
    }
    for (int k = 0; k < kTrainOutputs; ++k) o[k] = b2[k];
    for (int j = 0; j < H; ++j)
        for (int k = 0; k < kTrainOutputs; ++k) o[k] = o[k] + rh[j] * w2[j * kTrainOutputs + k];
    float mx = o[first];
    for (int a = first + 1; a < kActions; ++a)
        if (in_c[a]) mx = o[a] > mx ? o[a] : mx;
    float s = 0.0f;
    for (int a = 0; a < kActions; ++a) {
        if (!in_c[a]) continue;
        d[a] = o[a] - mx;
        e[a] = train_exp(d[a]);
        s = s + e[a];
    }
    const float L = train_log(s);
    float lp = 0.0f, lv, dv;
    for (int a = 0; a < kActions; ++a) {
        rdo[a] = 0.0f;
        if (!in_c[a]) continue;
        train_policy(e[a], s, d[a], L, A.visits[r * kActions + a], S, rdo[a], term[a]);
        lp = lp + term[a];
    }
    train_value(o[kActions], z, A.hy.value_reg, lv, dv);
    rdo[kActions] = dv;
    rdo[kTrainOutputs] = 0.0f;
    const float ww = EX && A.row_weight ? train_weight(A.row_weight[r]) : 1.0f;
    if (EX)
        for (int k = 0; k < kTrainOutputs; ++k) rdo[k] = ww * rdo[k];
    for (int j = 0; j < H; ++j) {
        float acc = 0.0f;
        for (int k = 0; k < kTrainOutputs; ++k) acc = acc + rdo[k] * w2[j * kTrainOutputs + k];
        rdh[j] = pre[j] > 0.0f ? acc : 0.0f;
    }
    if (EX) {
        if (A.row_loss_out) { A.row_loss_out[2 * r] = lp; A.row_loss_out[2 * r + 1] = lv; }
        if (A.prio_out) A.prio_out[r] = train_priority(lp, lv, A.prio_scale, A.prio_floor, A.prio_cap);
        rst[0] = ww * lp; rst[1] = ww * lv; rst[2] = top; rst[3] = 1.0f;
    } else {
        rst[0] = lp; rst[1] = lv; rst[2] = top; rst[3] = 1.0f;
    }
}

// SUM of the header over `len` neighbouring elements at once: term(r, acc) adds row r's terms to the chunk's accumulators
template <typename Term>
void train_sum(int64_t B, int len, float *total, Term term)
{
    GBL_FP_STRICT
    float acc[256];
    std::fill(total, total + len, 0.0f);
    for (int64_t r0 = 0; r0 < B; r0 += kTrainChunk) {
        std::fill(acc, acc + len, 0.0f);
        for (int64_t r = r0; r < std::min<int64_t>(B, r0 + kTrainChunk); ++r) term(r, acc);
        for (int i = 0; i < len; ++i) total[i] = total[i] + acc[i];
    }
}

// the step after the argument checks, for both entry points: the rows (EX: weighted, with the per-row outputs), then the row sums and Adam
template <bool EX>
int train_step_host(const HostTrain &A, int64_t B, float *params, float *adam_m, float *adam_v, float *grad_out, float *stats_out)
{
    GBL_FP_STRICT
    const int H = A.H;
    parallel_for(B, [=](int64_t r0, int64_t r1) {
        for (int64_t r = r0; r < r1; ++r) train_row<EX>(A, r);
    }, 64);
    int N = 0;
    for (int64_t r = 0; r < B; ++r) N += A.row[r * kTrainRowStats + 3] != 0.0f;
    const float M = (float)(N > 0 ? N : 1);
    // the segments of the parameter vector: the 117 rows of w1, b1, the H rows of w2, b2 -- each `len` neighbouring elements
    const int at_b1 = kObs * H, at_w2 = at_b1 + H, at_b2 = at_w2 + kTrainOutputs * H;
    parallel_for(kObs + 1 + H + 1, [=](int64_t s0, int64_t s1) {
        GBL_FP_STRICT
        float G[256];
        for (int64_t seg = s0; seg < s1; ++seg) {
            int at, len;
            if (seg < kObs) {
                const int f = (int)seg;
                at = f * H; len = H;
                train_sum(B, len, G, [&](int64_t r, float *acc) {
                    if (A.obs[r * kObs + f] == 0) return;
                    for (int j = 0; j < H; ++j) acc[j] = acc[j] + A.dh[r * H + j];
                });
            } else if (seg == kObs) {
                at = at_b1; len = H;
                train_sum(B, len, G, [&](int64_t r, float *acc) {
                    for (int j = 0; j < H; ++j) acc[j] = acc[j] + A.dh[r * H + j];
                });
            } else if (seg <= kObs + H) {
                const int j = (int)seg - kObs - 1;
                at = at_w2 + j * kTrainOutputs; len = kTrainOutputs;
                train_sum(B, len, G, [&](int64_t r, float *acc) {
                    for (int k = 0; k < kTrainOutputs; ++k) acc[k] = acc[k] + A.h[r * H + j] * A.dout[r * kTrainDoStride + k];
                });
            } else {
                at = at_b2; len = kTrainOutputs;
                train_sum(B, len, G, [&](int64_t r, float *acc) {
                    for (int k = 0; k < kTrainOutputs; ++k) acc[k] = acc[k] + A.dout[r * kTrainDoStride + k];
                });
            }
            for (int i = 0; i < len; ++i) {
                const float g = train_gradient(G[i], M, params[at + i], A.hy);
                train_adam(g, params[at + i], adam_m[at + i], adam_v[at + i], A.hy);
                if (grad_out) grad_out[at + i] = g;
            }
        }
    }, 8);
    float sums[2], top = 0.0f;
    train_sum(B, 2, sums, [&](int64_t r, float *acc) {
        GBL_FP_STRICT
        acc[0] = acc[0] + A.row[r * kTrainRowStats];
        acc[1] = acc[1] + A.row[r * kTrainRowStats + 1];
    });
    for (int64_t r = 0; r < B; ++r) {
        const float t = A.row[r * kTrainRowStats + 2];
        top = train_float_bits(t) > train_float_bits(top) ? t : top;
    }
    stats_out[0] = sums[0] / M; stats_out[1] = sums[1] / M; stats_out[2] = (float)N; stats_out[3] = top;
    return GBL_OK;
}

HostTrain host_train(const int8_t *obs, const int8_t *mask, const int16_t *visits, const int8_t *z, int64_t B, int H, const float *params,
                     const gbl_train_hyper *hyper, void *workspace)
{
    float *ws = static_cast<float *>(workspace);
    return HostTrain{obs, mask, visits, z, params, ws, ws + B * H, ws + 2 * B * H, ws + 2 * B * H + B * kTrainDoStride, H,
                     TrainHyper{hyper->lr, hyper->beta1, hyper->beta2, hyper->eps, hyper->weight_decay, hyper->value_reg, hyper->bias1,
                                hyper->bias2},
                     nullptr, nullptr, nullptr, 0.0f, 0, 0};
}

}  // namespace

extern "C" int gbl_cpu_train_step(const int8_t *obs, const int8_t *mask, const int16_t *visits, const int8_t *z, int64_t batch, int hidden,
                                  float *params, float *adam_m, float *adam_v, const gbl_train_hyper *hyper, float *grad_out,
                                  float *stats_out, void *workspace, int64_t workspace_bytes, void *)
{
    if (const char *why = train_error(obs, visits, z, batch, hidden, params, adam_m, adam_v, hyper, stats_out, workspace, workspace_bytes))
        return fail(GBL_ERR_ARG, why);
    return train_step_host<false>(host_train(obs, mask, visits, z, batch, hidden, params, hyper, workspace), batch, params, adam_m, adam_v,
                                  grad_out, stats_out);
}

// gbl_cpu_train_step_weighted: the same step with the rows' weights folded into do and the loss terms, and the two per-row outputs
extern "C" int gbl_cpu_train_step_weighted(const int8_t *obs, const int8_t *mask, const int16_t *visits, const int8_t *z, int64_t batch,
                                           int hidden, float *params, float *adam_m, float *adam_v, const gbl_train_hyper *hyper,
                                           const float *row_weight, float *row_loss_out, int32_t *prio_out, float prio_scale,
                                           int32_t prio_floor, int32_t prio_cap, float *grad_out, float *stats_out, void *workspace,
                                           int64_t workspace_bytes, void *)
{
    if (const char *why = train_error(obs, visits, z, batch, hidden, params, adam_m, adam_v, hyper, stats_out, workspace, workspace_bytes))
        return fail(GBL_ERR_ARG, why);
    if (const char *why = train_weighted_error(prio_out, prio_scale, prio_floor, prio_cap)) return fail(GBL_ERR_ARG, why);
    HostTrain A = host_train(obs, mask, visits, z, batch, hidden, params, hyper, workspace);
    A.row_weight = row_weight; A.row_loss_out = row_loss_out; A.prio_out = prio_out;
    A.prio_scale = prio_scale; A.prio_floor = prio_floor; A.prio_cap = prio_cap;
    return train_step_host<true>(A, batch, params, adam_m, adam_v, grad_out, stats_out);
}

// gbl_cpu_replay_importance: the header's rule, the integer minimum first
extern "C" int gbl_cpu_replay_importance(const int32_t *prio, int64_t batch, float beta, float *weights_out, void *)
{
    if (const char *why = replay_importance_error(prio, batch, beta, weights_out)) return fail(GBL_ERR_ARG, why);
    int32_t wmin = INT32_MAX;
    for (int64_t j = 0; j < batch; ++j)
        if (prio[j] > 0 && prio[j] < wmin) wmin = prio[j];
    for (int64_t j = 0; j < batch; ++j) weights_out[j] = importance_weight(prio[j], wmin, beta);
    return GBL_OK;
}
