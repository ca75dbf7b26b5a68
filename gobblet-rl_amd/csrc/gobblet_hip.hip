// gobblet_hip.hip -- gfx950 kernels + the C-ABI of include/gobblet_hip.h.
// Building blocks and the execution shape are described in gobblet_device.h.
#include "gobblet_device.h"

#include <stdio.h>
#include <algorithm>
#include <type_traits>
#include <utility>
#include <stdlib.h>
#include <string.h>

#include "../../include/gobblet_hip.h"
#include "gobblet_diag.h"
#include "gobblet_knobs.h"  // the product's constants -- or, in an experiment build (-DGBL_AB_BUILD), the A/B knobs of gobblet_ab.h

using namespace gbl;

namespace {

thread_local char g_err[256] = "";

int fail(int code, const char *msg)
{
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}

int hip_fail(hipError_t e, const char *what)
{
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return GBL_ERR_HIP;
}

// whether any of the pointers is off a `bytes`-byte boundary (a power of two); NULL adds nothing
template <typename... P>
inline bool off(uintptr_t bytes, const P *...p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & (bytes - 1)) != 0; }

struct Geometry {
    int64_t ntiles;
    uint32_t grid;
};

// waves: wavefronts per workgroup, each with a tile of its own (the step kernels; see kStepWaves)
inline Geometry geometry(int64_t n, int waves = 1)
{
    Geometry g;
    g.ntiles = (n + kTile - 1) / kTile;
    int64_t groups = (g.ntiles + waves - 1) / waves;
    int64_t chunk = (groups + 7) / 8;
    g.grid = (uint32_t)(chunk * 8);
    return g;
}

// blocks of nt tiles per workgroup (the greedy kernels): ntiles counts TILES, the grid blocks
inline Geometry block_geometry(int64_t n, int nt)
{
    Geometry g;
    g.ntiles = (n + kTile - 1) / kTile;
    const int64_t blocks = (g.ntiles + nt - 1) / nt;
    g.grid = (uint32_t)(((blocks + 7) / 8) * 8);
    return g;
}

// Wavefronts per workgroup of the step kernels.  The wavefronts of a workgroup are independent (a tile and an LDS
// image each, no barrier); a workgroup is only the unit of dispatch.
constexpr int kStepWaves = 1;  // (128- and 256-thread workgroups: +-1-2 %, round 1)

// Non-temporal store policy of the step kernels (see store_rows): stream the observation always, the
// mask too once one ply's footprint exceeds the 256 MiB Infinity Cache.  A pure function of the batch size: the
// library reads no environment and keeps no state (experiment builds pin a policy: gobblet_ab.h).
inline int nt_policy(int64_t n)
{
    if (knob::kForcedNt) return knob::kForcedNt == 3 ? 3 : 1;
    return n * 234 > ((int64_t)256 << 20) ? 3 : 1;
}

// gbl_collect always stores its trajectory rows non-temporally.  Plain (cached) stores win 5-12 % where the trajectory fits
// the Infinity Cache AND the batch is 131 072 - 262 144 boards, but lose 15 % at 65 536 boards and 30 % once it does not fit
// (see k_collect): the product build has no such path (experiment builds: gobblet_ab.h).

// Which kernel a gbl_collect call runs (also reported by gbl_collect_variant): GBL_COLLECT_PAIR = k_collect2 (grids of up
// to kCollect2MaxTiles tiles that stream), GBL_COLLECT_STREAM / GBL_COLLECT_CACHED = k_collect with non-temporal / plain
// stores.  A pure function of the call's shape (and of the -D macros of an A/B build).
// (round 5: the kernel needs 79 VGPRs since its ragged path stopped costing registers, and ten workgroups per CU are co-resident:
//  147 456 boards 4.08 against k_collect's 4.24 us per ply, 163 840: 4.39 / 4.53; 196 608 = 3 072 tiles: 5.67 / 5.30 -- until then
//  the limit was 2 048 tiles, eight workgroups of 122 VGPRs per CU)
constexpr int64_t kCollect2MaxTiles = 2560;

// Which form of the role kernel (k_collect_small<LA, KO, MERGE>, see there) a batch of n boards runs, as 100 LA + 10 KO + MERGE;
// 0 = none (k_collect2 / k_collect).  Measured, us per ply, FULL outputs, 32 plies per launch (scripts/experiments/ab_roles.sh, round 5):
// see the table in DESIGN.md 5.2.

// k_collect's occupancy, pinned: FOUR wavefronts per SIMD.  Until round 5 that was an accident of the register allocation (111
// VGPRs, most of them the ragged tile's byte loop's); when the ragged paths were rewritten the kernel needed 83, a fifth wavefront
// fitted, and the 2^20-board launch lost 2 % (27.19 -> 27.69 us per ply at 8 plies per launch, 26.86 -> 27.49 at 20; min 3 / max 3:
// 27.21 / 26.81; profiles/r05/collect_occupancy.txt) -- more tiles open at once is more write streams for the same DRAM pages.
constexpr int64_t kTrioHandMaxTiles = 8192;  // k_collect3<..., HAND>: the first row wavefront stores the scalars up to 524 288 boards


inline int small_cfg(int64_t n, bool with_mask, bool with_obs)
{
    (void)with_mask;
    if (knob::collect_cfg_override() >= 0) return knob::collect_cfg_override();  // (experiment builds only)
    if (knob::kForcedCollectSmall >= 0) return knob::kForcedCollectSmall;
    // (round 5, scripts/experiments/ab_roles.sh; DESIGN.md 5.2 has the table; 3 = k_collect3)
    // MASK_ONLY is bound by what ONE wavefront issues, so the player + mask-row pair of k_collect3 keeps paying far
    // into the HBM regime: 163 840 boards 1.79 against k_collect's 2.19 us per ply, 2^20: 10.39 against 10.93, 2^21: 19.9 against
    // 20.7; 2^22: 45.1 against 44.5 (profiles/r05/ab_roles_long_launches.txt)
    // (round 6: k_collect5 -- 32-board groups behind a hand-over ring, cfg 6 -- wherever its wavefronts find a SIMD each: MASK_ONLY 4 096 /
    //  8 192 boards 0.418 / 0.419 us per ply against the role kernel's 0.546 / 0.548, 16 384 ... 32 768: 0.50-0.55 against k_collect3's
    //  0.58-0.65, 49 152: 0.81 against 0.73; it needs the mask rows' wavefront: profiles/r06/ab_group32.txt)
    if (!with_obs) return n <= 32768 && with_mask ? 6 : n <= 8192 ? 210 : n <= 3 * (int64_t)(1 << 20) ? 3 : 0;
    // (with the trajectory arrays placed across HBM's memory classes: 40 960 boards k_collect3 1.31 against k_collect2's 1.40 us per
    //  ply, 49 152: 1.49 against 1.41 -- profiles/r05/placed_forms.txt)
    // (late round 5: with its scalars stored by the first row wavefront k_collect3 runs 0.634 us per ply at 8 192 ... 16 384 boards,
    //  256 plies per launch -- <1,2>: 0.643 at 12 288, 0.72 at 16 384; <2,2>: 0.558 at 8 192: profiles/r05/ab_trio_scalars.txt)
    // (round 6: FULL 4 096 / 8 192 boards k_collect5 0.440 / 0.439 us per ply against the role kernel's 0.525 / 0.527, 9 216: 0.59 against
    //  k_collect3's 0.63, 10 240: a tie -- from 257 groups on two of them share a CU)
    if (with_mask && n <= 9216) return 6;
    return n <= 8192 ? 220 : n <= 45056 ? 3 : 0;
}

inline int collect_variant(int64_t n, uint32_t plies, bool with_mask, bool with_obs)
{
    (void)plies;
    const bool nt = knob::kForcedCollectNt != 0;
    const bool pair = knob::kForcedCollectPair >= 0 ? knob::kForcedCollectPair != 0
                                                    : (n + kTile - 1) / kTile <= kCollect2MaxTiles && nt && (with_mask || with_obs);
    const int cfg = nt ? small_cfg(n, with_mask, with_obs) : 0;
    if (cfg == 3) return (with_mask || with_obs) ? GBL_COLLECT_TRIO : GBL_COLLECT_STREAM;
    if (cfg == 6) return with_mask ? GBL_COLLECT_GROUP32 : with_obs ? GBL_COLLECT_TRIO : GBL_COLLECT_STREAM;  // k_collect5 (needs the mask rows' wavefront)
    return cfg ? GBL_COLLECT_ROLES(cfg / 100, (cfg / 10) % 10, cfg % 10) : pair ? GBL_COLLECT_PAIR : nt ? GBL_COLLECT_STREAM : GBL_COLLECT_CACHED;
}

// LDS words for a tile image of ROWB-byte rows (+ slack for row_load's look-ahead dword)
template <int ROWB>
constexpr int image_words() { return kTile * ROWB / 4 + 4; }

// A wavefront's index in its workgroup, as a SCALAR: threadIdx.x >> 6 is the same on all lanes, but the compiler does not know it
// and keeps everything derived from it -- the tile index, every tile base address, the role tests -- in vector registers (in
// gbl_collect_policy: 64-bit per-lane addresses of seven output arrays, hoisted out of the ply loop and spilled to scratch).
__device__ __forceinline__ int wave_index()
{
#ifndef GBL_HOST_EMU
    return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#else
    return (int)(threadIdx.x >> 6);
#endif
}

// -------------------------------------------------------------------------------------------
// Per-lane state of one board inside a kernel.
struct Lane {
    int64_t tile, b;
    int lane, rows;
    bool valid;
};

template <int W = 1, bool XCD_REMAP = true>
__device__ __forceinline__ bool lane_setup(Lane &L, int64_t n, int64_t ntiles)
{
    if (W == 1) {
        L.tile = XCD_REMAP ? xcd_tile(blockIdx.x, ntiles) : (int64_t)blockIdx.x;
        L.lane = threadIdx.x;
    } else {  // W consecutive tiles per workgroup, one per wavefront
        L.tile = xcd_tile(blockIdx.x, (ntiles + W - 1) / W) * W + (threadIdx.x >> 6);
        L.lane = threadIdx.x & 63;
    }
    if (L.tile >= ntiles) return false;
    int64_t left = n - L.tile * kTile;
    L.rows = left < kTile ? (int)left : kTile;
    L.valid = L.lane < L.rows;
    L.b = L.tile * kTile + L.lane;
    return true;
}

// A wavefront's tallies of finished games and of each player's wins (ballot + popcount: wave-uniform) into the counters: one stripe
// (its own 128-byte line) per tile mod GBL_COUNTER_STRIPES, so that the device-scope atomics of concurrently finishing waves go to
// different lines.  (One lane calls it.)
__device__ __forceinline__ void tally_flush(int64_t *counters, int64_t stripe, int boards, uint32_t plies, uint32_t games, uint32_t w1,
                                            uint32_t w2)
{
    unsigned long long *c = reinterpret_cast<unsigned long long *>(counters) + (size_t)(stripe % GBL_COUNTER_STRIPES) * GBL_COUNTER_STRIDE;
    atomicAdd(c + 0, (unsigned long long)boards * plies);
    if (games) atomicAdd(c + 1, (unsigned long long)games);
    if (w1) atomicAdd(c + 2, (unsigned long long)w1);
    if (w2) atomicAdd(c + 3, (unsigned long long)w2);
}

template <typename Between = NoWork>
__device__ __forceinline__ void load_state(const int8_t *state, uint32_t *img, const Lane &L, uint32_t (&r)[7],
                                           Between between = Between())
{
    tile_in<kCells>(state + L.tile * (kTile * kCells), img, L.lane, L.rows, between);
    wave_lds_fence();
    row_load<kCells>(img, L.lane, r);
    r[6] &= 0x00FFFFFFu;  // (lanes past the end of a ragged last tile hold whatever the image held: see planes_of)
}

// The board's bit planes; lanes past the end of a ragged last tile get an EMPTY board (one select on the occupancy
// plane -- the other two are only read where it is set -- instead of seven on the row's dwords).  Nothing such a
// lane computes is ever stored: ragged tiles are written back byte-granular, valid rows only.
__device__ __forceinline__ Planes planes_of(const Lane &L, const uint32_t (&r)[7])
{
    Planes p = make_planes(r);
    p.nz = L.valid ? p.nz : 0u;
    return p;
}

// A lane's 54 mask bytes into its row of a tile's LDS image.  STAGED: the row is shifted onto aligned dwords in registers
// (row_stage: ~45 v_alignbyte / select instructions and a DPP fetch of the neighbour's bytes), every LDS access an aligned dword.
// Otherwise: 14 nibble expansions and four UNALIGNED LDS stores (rows are 2-byte aligned; gfx950 takes them) -- 45 VALU
// instructions less, more LDS passes.  Measured (round 5, profiles/r05/ab_maskrow.txt): the one-wavefront kernels, which are bound
// by what ONE wavefront issues, gain -- k_collect MASK_ONLY at 2^20 boards 10.88 -> 10.06 us per ply (0.80 -> 0.87 of the HBM peak),
// FULL and the one-ply kernels +-1 % -- while k_collect2, whose storing wavefront reads the image back beside the player's writes,
// loses (MASK_ONLY 0.92 -> 1.13 us per ply at 65 536 boards, 1.39 -> 1.69 at 131 072): it and the greedy kernels stay staged.
template <bool STAGED>
__device__ __forceinline__ void mask_to_image(uint32_t *img, int lane, uint64_t bits)
{
    if constexpr (STAGED) {
        uint32_t d[14];
        mask_row(bits, d);
        row_stage<kActions>(img, lane, d);
    } else {
        mask_row_part<1>(reinterpret_cast<uint8_t *>(img) + lane * kActions, bits, 0);
    }
}

// -------------------------------------------------------------------------------------------
// Board-level kernels (one reference function each)

__global__ __launch_bounds__(64) void k_legal_mask(const int8_t *__restrict__ state, const int8_t *__restrict__ to_move,
                                                   int8_t *__restrict__ mask, int64_t n, int64_t ntiles)
{
    __shared__ uint32_t s_state[image_words<kCells>()];
    __shared__ uint32_t s_mask[image_words<kActions>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    uint32_t r[7];
    load_state(state, s_state, L, r);
    Planes p = planes_of(L, r);
    int mover = L.valid ? to_move[L.b] : 0;
    mask_to_image<false>(s_mask, L.lane, legal54(p, mover != 0));
    wave_lds_fence();
    tile_out<kActions>(mask + L.tile * (kTile * kActions), s_mask, L.lane, L.rows);
}

__global__ __launch_bounds__(64) void k_is_legal(const int8_t *__restrict__ state, const int8_t *__restrict__ agent,
                                                 const int32_t *__restrict__ actions, int8_t *__restrict__ out,
                                                 int64_t n, int64_t ntiles)
{
    __shared__ uint32_t s_state[image_words<kCells>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    uint32_t r[7];
    load_state(state, s_state, L, r);
    if (!L.valid) return;
    Planes p = planes_of(L, r);
    int a = actions[L.b];
    uint64_t m = legal54(p, agent[L.b] != 0);
    bool ok = (uint32_t)a < (uint32_t)kActions && ((m >> (a & 63)) & 1ull);
    out[L.b] = ok ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_play_turn(int8_t *__restrict__ state, const int8_t *__restrict__ agent,
                                                  const int32_t *__restrict__ actions, int64_t n, int64_t ntiles)
{
    __shared__ uint32_t s_state[image_words<kCells>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    uint32_t r[7];
    load_state(state, s_state, L, r);
    Planes p = planes_of(L, r);
    int a = L.valid ? actions[L.b] : 0;
    int mover = L.valid ? (agent[L.b] != 0) : 0;
    uint64_t m = legal54(p, mover);
    bool ok = L.valid && (uint32_t)a < (uint32_t)kActions && ((m >> (a & 63)) & 1ull);
    if (ok) apply_move(p, r, mover, (uint32_t)a);
    row_stage<kCells>(s_state, L.lane, r);
    wave_lds_fence();
    tile_out<kCells>(state + L.tile * (kTile * kCells), s_state, L.lane, L.rows);
}

__global__ __launch_bounds__(64) void k_winner(const int8_t *__restrict__ state, int8_t *__restrict__ winner, int64_t n,
                                               int64_t ntiles)
{
    __shared__ uint32_t s_state[image_words<kCells>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    uint32_t r[7];
    load_state(state, s_state, L, r);
    if (!L.valid) return;
    winner[L.b] = (int8_t)winner_of(planes_of(L, r));
}

__global__ __launch_bounds__(64) void k_flatboard(const int8_t *__restrict__ state, int8_t *__restrict__ flat, int64_t n,
                                                  int64_t ntiles)
{
    __shared__ uint32_t s_state[image_words<kCells>()];
    __shared__ uint32_t s_flat[image_words<9>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    uint32_t r[7];
    load_state(state, s_state, L, r);
    uint32_t d[3];
    flat_row(planes_of(L, r), r, d);
    row_stage<9>(s_flat, L.lane, d);
    wave_lds_fence();
    tile_out<9>(flat + L.tile * (kTile * 9), s_flat, L.lane, L.rows);
}

__global__ __launch_bounds__(64) void k_covered(const int8_t *__restrict__ state, int8_t *__restrict__ cov, int64_t n,
                                                int64_t ntiles)
{
    __shared__ uint32_t s_state[image_words<kCells>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    uint32_t r[7];
    load_state(state, s_state, L, r);
    uint32_t d[7];
    covered_row(planes_of(L, r), d);
    wave_lds_fence();  // every lane has read its row before the image is reused
    row_stage<kCells>(s_state, L.lane, d);
    wave_lds_fence();
    tile_out<kCells>(cov + L.tile * (kTile * kCells), s_state, L.lane, L.rows);
}

__global__ __launch_bounds__(64) void k_observe(const int8_t *__restrict__ state, const int8_t *__restrict__ to_move,
                                                int agent_sel, int8_t *__restrict__ obs, int64_t n, int64_t ntiles)
{
    __shared__ uint32_t s_state[image_words<kCells>()];
    __shared__ uint32_t s_obs[image_words<kObs>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    uint32_t r[7];
    load_state(state, s_state, L, r);
    int who = agent_sel >= 0 ? agent_sel : (L.valid ? to_move[L.b] : 0);
    obs_image_zero(s_obs, L.lane);
    wave_lds_fence();
    obs_scatter(s_obs, L.lane, planes_of(L, r), who != 0);
    wave_lds_fence();
    tile_out<kObs, kStoreStreamDrop>(obs + L.tile * (kTile * kObs), s_obs, L.lane, L.rows);
}

// gbl_board_eval: optional Board.play_turn, then one record per board with everything the reference derives
// from the position (the seven board-level kernels above in one launch; the single-environment facade's ply).
// Every field of a record starts on a dword, records are 432 bytes apart, so a lane writes its record into
// the LDS image with plain dword stores; the observations are scattered sparsely as in k_observe.
static_assert(GBL_REC_BYTES % 16 == 0 && GBL_REC_OBS1 + kObs <= GBL_REC_BYTES, "record layout");
static_assert(GBL_REC_SQUARES % 4 == 0 && GBL_REC_WINNER % 4 == 0 && GBL_REC_FLAT % 4 == 0 && GBL_REC_COVERED % 4 == 0 &&
              GBL_REC_MASK0 % 4 == 0 && GBL_REC_MASK1 % 4 == 0 && GBL_REC_OBS0 % 4 == 0 && GBL_REC_OBS1 % 4 == 0,
              "record fields are dword aligned");

__global__ __launch_bounds__(64) void k_board_eval(int8_t *__restrict__ state, const int8_t *__restrict__ agent,
                                                   const int32_t *__restrict__ actions, int8_t *__restrict__ rec,
                                                   int64_t n, int64_t ntiles)
{
    __shared__ uint32_t s_state[image_words<kCells>()];
    __shared__ uint32_t s_rec[image_words<GBL_REC_BYTES>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    uint32_t r[7];
    load_state(state, s_state, L, r);
    Planes p = planes_of(L, r);
    if (actions) {  // board.py:118-132
        const int a = L.valid ? actions[L.b] : -1;
        const int mover = L.valid ? (agent[L.b] != 0) : 0;
        const uint64_t m = legal54(p, mover);
        if ((uint32_t)a < (uint32_t)kActions && ((m >> (a & 63)) & 1ull)) apply_move(p, r, mover, (uint32_t)a);
        wave_lds_fence();  // every lane has read its row before the image is rebuilt
        row_stage<kCells>(s_state, L.lane, r);
        wave_lds_fence();
        tile_out<kCells>(state + L.tile * (kTile * kCells), s_state, L.lane, L.rows);
    }
    {  // zero the record image (padding bytes and the observation planes' zeros)
        constexpr int NV = kTile * GBL_REC_BYTES / 16;
        static_assert(NV % 64 == 0, "whole vectors per lane");
        uint4 *lv = reinterpret_cast<uint4 *>(s_rec);
        const uint4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < NV / 64; ++i) lv[L.lane + 64 * i] = z;
    }
    wave_lds_fence();
    uint32_t *row = s_rec + L.lane * (GBL_REC_BYTES / 4);
    r[6] &= 0x00FFFFFFu;
#pragma unroll
    for (int j = 0; j < 7; ++j) row[GBL_REC_SQUARES / 4 + j] = r[j];
    row[GBL_REC_WINNER / 4] = (uint32_t)winner_of(p) & 0xFFu;
    uint32_t f[3], c[7], m0[14], m1[14];
    flat_row(p, r, f);
    covered_row(p, c);
    mask_row(legal54(p, 0), m0);
    mask_row(legal54(p, 1), m1);
#pragma unroll
    for (int j = 0; j < 3; ++j) row[GBL_REC_FLAT / 4 + j] = f[j];
#pragma unroll
    for (int j = 0; j < 7; ++j) row[GBL_REC_COVERED / 4 + j] = c[j];
#pragma unroll
    for (int j = 0; j < 14; ++j) {
        row[GBL_REC_MASK0 / 4 + j] = m0[j];
        row[GBL_REC_MASK1 / 4 + j] = m1[j];
    }
    obs_scatter_row(reinterpret_cast<uint8_t *>(row) + GBL_REC_OBS0, p, 0);
    obs_scatter_row(reinterpret_cast<uint8_t *>(row) + GBL_REC_OBS1, p, 1);
    wave_lds_fence();
    // records out: 16-byte vectors, four in flight per lane (tile_out would hold all 27 in registers)
    const int nv = L.rows * (GBL_REC_BYTES / 16);
    uint4 *gv = reinterpret_cast<uint4 *>(rec + L.tile * (int64_t)(kTile * GBL_REC_BYTES));
    const uint4 *lv = reinterpret_cast<const uint4 *>(s_rec);
    for (int i0 = 0; i0 < nv; i0 += 256) {
        uint4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = lv[min(i0 + 64 * u + L.lane, nv - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + 64 * u + L.lane < nv) gv[i0 + 64 * u + L.lane] = v[u];
    }
}

// Rows of a tile -> HBM through ONE LDS image that is reused.  On entry it holds the tile's state rows
// where the load put them, already patched by the plies (ImageRow): they go out as they are.  Then the
// image is free (the LDS reads of tile_out are issued before the next writes) for the 117-byte
// observation rows, and after those for the mask rows.  7.5 KB of LDS per wave instead of 12.7 KB: more
// resident waves per CU to cover the store latency.
template <bool WITH_MASK, bool WITH_OBS>
constexpr int out_image_words()
{
    return WITH_OBS ? image_words<kObs>() : WITH_MASK ? image_words<kActions>() : image_words<kCells>();
}
static_assert(image_words<kObs>() >= image_words<kActions>() && image_words<kActions>() >= image_words<kCells>(),
              "the largest row stream of a variant sizes its image");
static_assert(image_words<kObs>() % 4 == 0 && image_words<kActions>() % 4 == 0 && image_words<kCells>() % 4 == 0,
              "images of the wavefronts of a workgroup lie back to back, 16-byte aligned");

// NT: which row streams are stored with the non-temporal hint -- bit 0 observation, bit 1 mask, bit 2
// state.  Measured (profiles/r01): the write-once observation stream always gains from it; the mask
// stream gains once a ply's footprint (234 B per board) no longer fits the 256 MiB Infinity Cache
// (2^22 boards: 169 -> 141 us) and loses ~2 % below that; the state rows are re-read next ply and stay
// cached.  The host picks the variant from the batch size (nt_policy()).
// the tile's observation rows (raw_env.observe of `observer`) through the image `img`; obs_tile: the tile's first row
template <int NT>
__device__ __forceinline__ void store_obs(uint32_t *img, const Lane &L, const Planes &p, int observer,
                                          int8_t *__restrict__ obs_tile)
{
    obs_image_zero(img, L.lane);
    wave_lds_fence();
    obs_scatter(img, L.lane, p, observer);
    wave_lds_fence();
    tile_out<kObs, NT>(obs_tile, img, L.lane, L.rows);
    wave_lds_fence();
}

// the tile's mask rows from 54-bit sets; mask_tile: the tile's first row
template <int NT>
__device__ __forceinline__ void store_mask(uint32_t *img, const Lane &L, uint64_t legal, int8_t *__restrict__ mask_tile)
{
    mask_to_image<false>(img, L.lane, legal);
    wave_lds_fence();
    tile_out<kActions, NT>(mask_tile, img, L.lane, L.rows);
    wave_lds_fence();
}

// Returns the 54-bit set behind the mask rows it stored (WITH_MASK; 0 otherwise): gbl_step_ex draws the next action from it.
template <bool WITH_MASK, bool WITH_OBS, int NT>
__device__ __forceinline__ uint64_t store_rows(uint32_t *img, const Lane &L, bool mask_zero, const Planes &p, int observer,
                                               int8_t *__restrict__ state, int8_t *__restrict__ mask_out,
                                               int8_t *__restrict__ obs_out)
{
    wave_lds_fence();  // every lane's byte patches are in the image
    tile_out<kCells, (NT & 4) ? kStoreStream : kStorePlain>(state + L.tile * (kTile * kCells), img, L.lane, L.rows);
    wave_lds_fence();
    if (WITH_OBS) store_obs<(NT & 1) ? kStoreStreamDrop : kStorePlain>(img, L, p, observer, obs_out + L.tile * (kTile * kObs));
    // the next mover's legal mask is computed only now, behind the state and observation stores: the
    // sooner a wave's first stores are in flight, the shorter the launch's ramp-up
    uint64_t legal = 0ull;
    if (WITH_MASK) {
        legal = mask_zero ? 0ull : legal54(p, observer);
        store_mask<(NT & 2) ? kStoreStreamDrop : kStorePlain>(img, L, legal, mask_out + L.tile * (kTile * kActions));
    }
    return legal;
}

// (GBL_STAMP* : per-wavefront phase stamps of the diagnostic build, gobblet_diag.h; they expand to nothing here)

// gbl_step: fused raw_env.step + observe(next mover) over a tile of boards.
// (argument order: what a wavefront needs first comes first -- the first 16 dwords are preloaded into SGPRs at
// wave launch, -amdgpu-kernarg-preload-count, so the tile loads do not wait for a kernel-argument fetch)
// EXT: gbl_step_into / gbl_step_ex -- the ply's scalars also go to a trajectory slot, the status byte of every action, and the
// NEXT mover's masked-uniform draw (the gbl_sample rule on the mask this launch stores: the sampler's own launch and its 58 bytes
// per board of traffic leave an external policy's pipeline).  A template parameter: as run-time tests of three more pointers the
// plain step paid 0.5 us at 2^20 boards.
struct StepExt {
    int32_t *actions_copy;
    int8_t *done_copy, *to_move_copy, *status;
    int32_t *next_actions;       // may alias `actions`: a lane reads its board's action before it writes the next one
    uint64_t seed, env_base;
    const uint32_t *ply_dev;
    uint32_t ply;                // the draw's ply index (+ *ply_dev)
};

template <bool WITH_MASK, bool WITH_OBS, int NT, bool EXT>
__global__ __launch_bounds__(64 * kStepWaves) void k_step(int8_t *__restrict__ state, int8_t *__restrict__ to_move,
                                             int8_t *__restrict__ done, const int32_t *actions,
                                             int64_t n, int64_t ntiles, int illegal_mode, int auto_reset,
                                             int8_t *__restrict__ winner_out, int8_t *__restrict__ reward_out,
                                             int8_t *__restrict__ mask_out, int8_t *__restrict__ obs_out,
                                             int32_t *__restrict__ turn, StepExt X)
{
    constexpr int kImg = out_image_words<WITH_MASK, WITH_OBS>();
    __shared__ uint32_t s_imgs[kStepWaves * kImg];
    uint32_t *const s_img = s_imgs + (kStepWaves > 1 ? (threadIdx.x >> 6) * kImg : 0);
    Lane L;
    if (!lane_setup<kStepWaves>(L, n, ntiles)) return;
    // Per-board scalars first, from a clamped index and with no branch around them (a branch would
    // pin their s_waitcnt to the load): they are in flight together with the tile's loads -- one HBM
    // round trip per wave instead of two.
    const int64_t bs = L.valid ? L.b : n - 1;
    int mover = to_move[bs], was_done = done[bs], action = actions[bs];
    uint32_t r[7];
    uint32_t word = 0;  // EXT: the next mover's 32 random bits -- they depend on nothing the tile holds, so they are drawn under its loads
    load_state(state, s_img, L, r, [&] {
        if (EXT && X.next_actions) {
            const uint32_t ply = X.ply + (X.ply_dev ? *X.ply_dev : 0u);
            word = draw32(X.seed, X.env_base + (uint64_t)L.b, ply);
        }
    });
    mover = L.valid && mover != 0;
    was_done = L.valid && !auto_reset && was_done != 0;
    action = L.valid ? action : 0;
    Planes p = planes_of(L, r);
    Ply y;
    int dn;
    step_lane(ImageRow{reinterpret_cast<uint8_t *>(s_img) + L.lane * kCells}, p, mover, was_done, action, illegal_mode,
              auto_reset, dn, y);
    // gobblet.py:209: the mask belongs to the agent to move; a frozen board has nobody to move
    const bool frozen = dn && !auto_reset;
    const uint64_t stored = store_rows<WITH_MASK, WITH_OBS, NT>(s_img, L, frozen, p, mover, state, mask_out, obs_out);
    if (L.valid) {
        to_move[L.b] = (int8_t)mover;
        done[L.b] = (int8_t)dn;
        if (winner_out) winner_out[L.b] = (int8_t)y.winner;
        if (reward_out)
            reinterpret_cast<uint16_t *>(reward_out)[L.b] = (uint16_t)((y.r0 & 0xFF) | ((y.r1 & 0xFF) << 8));
        if (turn) turn[L.b] = next_turn(turn[L.b], y, auto_reset);
        if (EXT) {
            if (X.actions_copy) X.actions_copy[L.b] = action;
            if (X.done_copy) X.done_copy[L.b] = (int8_t)dn;
            if (X.to_move_copy) X.to_move_copy[L.b] = (int8_t)mover;
            if (X.status) X.status[L.b] = (int8_t)(was_done ? 0 : action_status(y.ok, action));  // (a frozen board consumes no action)
            if (X.next_actions) {  // gbl_sample's rule on the mask just stored (-1 where nobody is to move)
                const uint64_t legal = WITH_MASK ? stored : (frozen ? 0ull : legal54(p, mover));
                X.next_actions[L.b] = pick54(legal, word);
            }
        }
    }
}

// gbl_rollout: `plies` masked-random plies (sample + step + auto-reset) per launch; the board lives
// in registers between plies and the outputs of the LAST ply are stored.  plies = 1 is the fused
// "sample + step" ply of the benchmark pipeline.
// DEV_PLY: the ply index is ply0 + *ply_dev (gbl_rollout_at, graph replay).  A template parameter because even
// the never-taken runtime test costs the by-value kernel 0.3 us: it sits in front of the hoisted draw.
// ONE_PLY: plies == 1 known at compile time (the fused ply of a ply-by-ply pipeline): no loop, no second draw.
template <bool WITH_MASK, bool WITH_OBS, int NT, bool DEV_PLY, bool ONE_PLY>
__global__ __launch_bounds__(64 * kStepWaves) void k_rollout(int8_t *__restrict__ state, int8_t *__restrict__ to_move,
                                                int64_t n, int64_t ntiles, uint64_t seed, uint64_t env_base,
                                                const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies,
                                                int8_t *__restrict__ done, int32_t *__restrict__ actions_out,
                                                int8_t *__restrict__ winner_out, int8_t *__restrict__ reward_out,
                                                int8_t *__restrict__ mask_out, int8_t *__restrict__ obs_out,
                                                int illegal_mode, int64_t *__restrict__ counters,
                                                int32_t *__restrict__ turn)
{
    constexpr int kImg = out_image_words<WITH_MASK, WITH_OBS>();
    __shared__ uint32_t s_imgs[kStepWaves * kImg];
    uint32_t *const s_img = s_imgs + (kStepWaves > 1 ? (threadIdx.x >> 6) * kImg : 0);
    GBL_STAMP(0);
    GBL_STAMP_REAL(0);
    if (DEV_PLY) ply0 += *ply_dev;
    Lane L;
    if (!lane_setup<kStepWaves>(L, n, ntiles)) return;
    int mover = to_move[L.valid ? L.b : n - 1];  // issued before the tile loads, branch-free (see k_step)
    uint32_t r[7];
    // The first ply's random draw does not depend on the board: it is computed while the tile's loads
    // are in flight (between their issue and the LDS commit), off the wave's serial path.
    Draw4 block{{0u, 0u, 0u, 0u}};
    load_state(state, s_img, L, r, [&] { block = draw_block(seed, env_base + (uint64_t)L.b, ply0); });
    mover = L.valid && mover != 0;
    GBL_STAMP_DEP(1, r[0] + (uint32_t)mover);
    Planes p = planes_of(L, r);
    const ImageRow row{reinterpret_cast<uint8_t *>(s_img) + L.lane * kCells};  // the board's row, patched in place
    uint32_t games = 0, w1 = 0, w2 = 0;  // wave-uniform tallies (ballot + popcount)
    Ply y{0, 0, 0, false, false};
    int dn = 0, action = -1, tcount = 0;  // tcount: turn delta, or the absolute turn once a reset happened
    bool treset = false;
    if (ONE_PLY) plies = 1;
    for (uint32_t t = 0; t < plies; ++t) {
        const uint32_t ply = ply0 + t;
        action = pick54(legal54(p, mover), draw_word(block, ply));
        if (!ONE_PLY && t + 1 < plies && ((ply + 1) & 3u) == 0) block = draw_block(seed, env_base + (uint64_t)L.b, ply + 1);
        step_lane(row, p, mover, 0, action, illegal_mode, 1, dn, y);
        tcount = next_turn(tcount, y, 1);
        treset = treset || y.terminal;
        if (counters) {
            games += __popcll(__ballot(L.valid && y.terminal));
            w1 += __popcll(__ballot(L.valid && y.winner == 1));
            w2 += __popcll(__ballot(L.valid && y.winner == -1));
        }
    }
    GBL_STAMP_DEP(2, p.nz + (uint32_t)action);
    store_rows<WITH_MASK, WITH_OBS, NT>(s_img, L, false, p, mover, state, mask_out, obs_out);
    GBL_STAMP(3);
    if (L.valid) {
        to_move[L.b] = (int8_t)mover;
        done[L.b] = (int8_t)dn;
        if (actions_out) actions_out[L.b] = action;
        if (winner_out) winner_out[L.b] = (int8_t)y.winner;
        if (reward_out)
            reinterpret_cast<uint16_t *>(reward_out)[L.b] = (uint16_t)((y.r0 & 0xFF) | ((y.r1 & 0xFF) << 8));
        if (turn) turn[L.b] = treset ? tcount : turn[L.b] + tcount;
    }
    // Tallies (tally_flush spelled out: through the helper this kernel's code changes -- the scheduler orders its zero-initialisations
    // differently)
    if (counters && L.lane == 0) {
        unsigned long long *c = reinterpret_cast<unsigned long long *>(counters) +
                                (size_t)(L.tile % GBL_COUNTER_STRIPES) * GBL_COUNTER_STRIDE;
        atomicAdd(c + 0, (unsigned long long)L.rows * plies);
        if (games) atomicAdd(c + 1, (unsigned long long)games);
        if (w1) atomicAdd(c + 2, (unsigned long long)w1);
        if (w2) atomicAdd(c + 3, (unsigned long long)w2);
    }
    GBL_STAMP(4);
    GBL_STAMP_DRAIN(5);
    GBL_STAMP_FLUSH(L.tile);
}

// gbl_collect: `plies` masked-random plies per launch with EVERY ply's outputs materialised -- ply t writes its
// action, winner, reward, done, next mover, legal mask and observation into slot t of trajectory arrays
// ([plies][slot_boards][...]), exactly what `plies` launches of gbl_rollout(plies = 1) with advancing output
// pointers leave behind.  The tile's state is loaded once, lives in its LDS image (patched per move) and in the
// lane's bit planes for all plies, and is stored once; a wavefront's stores of ply t drain while it computes
// ply t + 1, there is no kernel boundary, no launch ramp and no state traffic between plies, and the legal mask
// stored for the next mover is the one the next ply samples from (computed once).
// NT: the trajectory rows are stored with the non-temporal hint (a trajectory larger than the Infinity Cache is a
// write-once stream to HBM: 2^20 boards x 8 plies 34.6 vs 45.0 us per ply) or plainly (a trajectory that fits the
// 256 MiB cache stays there for whoever reads it next and is overwritten there by the next launch: 131 072 boards x 8
// plies 4.15 vs 4.76 us per ply, 262 144 x 4: 8.5 vs 9.5 -- but 65 536 x 16: 2.44 vs 2.12); the host decides by the
// footprint in A/B builds only (gpurun_out/ab5, scripts/sweep_sizes.py with -DGBL_FORCE_COLLECT_NT=0|1); the product streams.
template <bool WITH_MASK, bool WITH_OBS, bool DEV_PLY, bool NT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(GBL_KNOB_COLLECT_WAVES_PER_EU))) void k_collect(int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n,
                                                int64_t ntiles, uint64_t seed, uint64_t env_base,
                                                const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies,
                                                int8_t *__restrict__ done, int64_t ply_stride, int64_t tile_stride,
                                                int32_t *__restrict__ actions_t, int8_t *__restrict__ winner_t,
                                                int8_t *__restrict__ reward_t, int8_t *__restrict__ done_t,
                                                int8_t *__restrict__ to_move_t, int8_t *__restrict__ mask_t,
                                                int8_t *__restrict__ obs_t, int illegal_mode,
                                                int64_t *__restrict__ counters, int32_t *__restrict__ turn,
                                                const int32_t *__restrict__ first_actions, int8_t *__restrict__ first_status)
{
    __shared__ uint32_t s_state[image_words<kCells>()];
    __shared__ uint32_t s_out[out_image_words<true, WITH_OBS>()];
    GBL_STAMP(0);
    GBL_STAMP_REAL(0);
    if (DEV_PLY) ply0 += *ply_dev;
    Lane L;
    // identity block -> tile map: the trajectory is written once and streams to HBM, where ONE write front per
    // array beats eight (one per XCD) -- unlike the single-ply kernels, whose outputs are rewritten every launch
    if (!lane_setup<1, false>(L, n, ntiles)) return;
    int mover = to_move[L.valid ? L.b : n - 1];
    // gbl_collect_from: the first ply plays the caller's actions (an external policy), the others are sampled
    int given = first_actions ? first_actions[L.valid ? L.b : n - 1] : 0;
    uint32_t r[7];
    Draw4 block{{0u, 0u, 0u, 0u}};
    load_state(state, s_state, L, r, [&] { block = draw_block(seed, env_base + (uint64_t)L.b, ply0); });
    mover = L.valid && mover != 0;
    Planes p = planes_of(L, r);
    const ImageRow row{reinterpret_cast<uint8_t *>(s_state) + L.lane * kCells};
    uint32_t games = 0, w1 = 0, w2 = 0;
    Ply y{0, 0, 0, false, false};
    int dn = 0, tcount = 0;
    bool treset = false;
    uint64_t legal = legal54(p, mover);
    if (first_status && L.valid) first_status[L.b] = (int8_t)action_status_of(legal, given);  // (gbl_collect_from_ex; outside the ply loop)
    for (uint32_t t = 0; t < plies; ++t) {
        const uint32_t ply = ply0 + t;
        int action = pick54(legal, draw_word(block, ply));
        if (first_actions && t == 0) action = given;
        if (t + 1 < plies && ((ply + 1) & 3u) == 0) block = draw_block(seed, env_base + (uint64_t)L.b, ply + 1);
        {  // step_lane with the mover's mask at hand (a sampled action is legal by construction: only gbl_collect_from's given ones are tested)
            if (first_actions && t == 0) y = play_ply(p, row, mover, legal, action, illegal_mode);
            else y = play_ply<true>(p, row, mover, legal, action, illegal_mode);
            dn = y.terminal ? 1 : 0;
            if (y.terminal) {  // raw_env.reset, gobblet.py:275-290
                p = Planes{0u, 0u, 0u};
                mover = 0;
                row.reset();
            }
        }
        tcount = next_turn(tcount, y, 1);
        treset = treset || y.terminal;
        if (counters) {
            games += __popcll(__ballot(L.valid && y.terminal));
            w1 += __popcll(__ballot(L.valid && y.winner == 1));
            w2 += __popcll(__ballot(L.valid && y.winner == -1));
        }
        // ply t of this tile: boards [cell, cell + 64) of the trajectory arrays
        const int64_t cell = (int64_t)t * ply_stride + L.tile * tile_stride;
        if (L.valid) {
            const int64_t at = cell + L.lane;
            if (actions_t) actions_t[at] = action;
            if (winner_t) winner_t[at] = (int8_t)y.winner;
            if (reward_t) reinterpret_cast<uint16_t *>(reward_t)[at] = (uint16_t)((y.r0 & 0xFF) | ((y.r1 & 0xFF) << 8));
            if (done_t) done_t[at] = (int8_t)dn;
            if (to_move_t) to_move_t[at] = (int8_t)mover;
        }
        constexpr int kPolicy = NT ? kStoreStreamDrop : kStorePlain;
        if (WITH_OBS) store_obs<kPolicy>(s_out, L, p, mover, obs_t + cell * kObs);
        legal = legal54(p, mover);  // the next mover's: stored now, sampled from next ply
        if (WITH_MASK) store_mask<kPolicy>(s_out, L, legal, mask_t + cell * kActions);
    }
    wave_lds_fence();  // every lane's byte patches are in the state image
    tile_out<kCells>(state + L.tile * (kTile * kCells), s_state, L.lane, L.rows);
    if (L.valid) {
        to_move[L.b] = (int8_t)mover;
        done[L.b] = (int8_t)dn;
        if (turn) turn[L.b] = treset ? tcount : turn[L.b] + tcount;
    }
    if (counters && L.lane == 0) tally_flush(counters, L.tile, L.rows, plies, games, w1, w2);
    GBL_STAMP(1); GBL_STAMP(2); GBL_STAMP(3); GBL_STAMP(4);
    GBL_STAMP_DRAIN(5);
    GBL_STAMP_FLUSH(L.tile);
}

// gbl_collect for grids that fit the chip in one batch (up to kCollect2MaxTiles tiles): TWO wavefronts per tile.  A
// wavefront whose stores are held back at issue cannot compute, and with eight or sixteen wavefronts per CU all in step
// nothing else fills the gap (the think-time model).  So the roles are dealt out: wavefront 0 plays the
// game -- pick, move, winner, auto-reset, tallies, the observation image, the next mask, its image -- and never
// issues a trajectory store; wavefront 1 takes the finished images over into registers (after which wavefront 0
// rebuilds them for the next ply; the observation image comes back zeroed) and does nothing but store.  Two barriers per ply: "images ready" and "images
// taken".  Bit for bit the trajectories of k_collect.
template <bool WITH_MASK, bool WITH_OBS, bool DEV_PLY>
__global__ __launch_bounds__(128) void k_collect2(int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n,
                                                 int64_t ntiles, uint64_t seed, uint64_t env_base,
                                                 const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies,
                                                 int8_t *__restrict__ done, int64_t ply_stride, int64_t tile_stride,
                                                 int32_t *__restrict__ actions_t, int8_t *__restrict__ winner_t,
                                                 int8_t *__restrict__ reward_t, int8_t *__restrict__ done_t,
                                                 int8_t *__restrict__ to_move_t, int8_t *__restrict__ mask_t,
                                                 int8_t *__restrict__ obs_t, int illegal_mode,
                                                 int64_t *__restrict__ counters, int32_t *__restrict__ turn,
                                                 const int32_t *__restrict__ first_actions, int8_t *__restrict__ first_status)
{
    __shared__ uint32_t s_state[image_words<kCells>()];
    __shared__ uint32_t s_obs[WITH_OBS ? image_words<kObs>() : 4];
    __shared__ uint32_t s_mask[WITH_MASK ? image_words<kActions>() : 4];
    __shared__ uint32_t s_small[kTile][2];  // per board: the action; winner | reward << 8 | done << 24 | to_move << 25
    if (DEV_PLY) ply0 += *ply_dev;
    // (Round 5 tried to alternate the playing wavefront between the workgroups that share a CU -- wavefront 0 in workgroups w and
    //  w + 256, wavefront 1 in w + 512 and w + 768 -- on the theory that all players of a CU sit on two of its four SIMDs: WORSE,
    //  MASK_ONLY 0.92 -> 1.16 us per ply at 65 536 boards, 1.29 -> 1.91 at 131 072; FULL +0 ... +6 %: profiles/r05/pair_flip.txt.)
    const int role = wave_index();
    Lane L;
    L.tile = (int64_t)blockIdx.x;
    L.lane = threadIdx.x & 63;
    if (L.tile >= ntiles) return;  // (the same for both wavefronts of the workgroup)
    const int64_t left = n - L.tile * kTile;
    L.rows = left < kTile ? (int)left : kTile;
    L.valid = L.lane < L.rows;
    L.b = L.tile * kTile + L.lane;
    constexpr int kPolicy = kStoreStreamDrop;
    if (role == 1) {
        // ---- the storing wavefront ---------------------------------------------------------------------------------
        for (uint32_t t = 0; t < plies; ++t) {
            const int64_t cell = (int64_t)t * ply_stride + L.tile * tile_stride;
            uint4 vo[kTile * kObs / 16 / 64 + 1], vm[kTile * kActions / 16 / 64 + 1];
            pair_barrier();  // images ready
            const uint32_t act = s_small[L.lane][0], sc = s_small[L.lane][1];
            if (WITH_OBS) tile_fetch<kObs>(s_obs, L.lane, vo);
            if (WITH_MASK) tile_fetch<kActions>(s_mask, L.lane, vm);
            if (L.rows != kTile) {  // the ragged last tile: the last few bytes of its rows straight from the images, now
                if (WITH_OBS) sub_tail(obs_t + cell * kObs, s_obs, L.lane, L.rows * kObs);
                if (WITH_MASK) sub_tail(mask_t + cell * kActions, s_mask, L.lane, L.rows * kActions);
            }
            if (WITH_OBS) {  // hand the observation image back zeroed: off the playing wavefront's path
                wave_lds_fence();
                obs_image_zero(s_obs, L.lane);
            }
            pair_barrier();  // images taken
            if (L.valid) {
                const int64_t at = cell + L.lane;
                if (actions_t) actions_t[at] = (int32_t)act;
                if (winner_t) winner_t[at] = (int8_t)(sc & 0xFFu);
                if (reward_t) reinterpret_cast<uint16_t *>(reward_t)[at] = (uint16_t)((sc >> 8) & 0xFFFFu);
                if (done_t) done_t[at] = (int8_t)((sc >> 24) & 1u);
                if (to_move_t) to_move_t[at] = (int8_t)((sc >> 25) & 1u);
            }
            // (a ragged tile: the whole vectors of its rows -- the descriptor ends there)
            if (WITH_OBS) tile_store<kObs, kPolicy>(obs_t + cell * kObs, vo, L.lane, (L.rows * kObs) & ~15);
            if (WITH_MASK) tile_store<kActions, kPolicy>(mask_t + cell * kActions, vm, L.lane, (L.rows * kActions) & ~15);
        }
        return;
    }
    // ---- the playing wavefront (k_collect's loop without its trajectory stores) -------------------------------------
    int mover = to_move[L.valid ? L.b : n - 1];
    int given = first_actions ? first_actions[L.valid ? L.b : n - 1] : 0;  // (gbl_collect_from, see k_collect)
    uint32_t r[7];
    Draw4 block{{0u, 0u, 0u, 0u}};
    load_state(state, s_state, L, r, [&] { block = draw_block(seed, env_base + (uint64_t)L.b, ply0); });
    mover = L.valid && mover != 0;
    Planes p = planes_of(L, r);
    const ImageRow row{reinterpret_cast<uint8_t *>(s_state) + L.lane * kCells};
    uint32_t games = 0, w1 = 0, w2 = 0;
    Ply y{0, 0, 0, false, false};
    int dn = 0, tcount = 0;
    bool treset = false;
    uint64_t legal = legal54(p, mover);
    if (first_status && L.valid) first_status[L.b] = (int8_t)action_status_of(legal, given);  // (gbl_collect_from_ex)
    if (WITH_OBS) {  // the first ply's observation image (later ones come back zeroed from the storing wavefront)
        obs_image_zero(s_obs, L.lane);
        wave_lds_fence();
    }
    for (uint32_t t = 0; t < plies; ++t) {
        const uint32_t ply = ply0 + t;
        int action = pick54(legal, draw_word(block, ply));
        if (first_actions && t == 0) action = given;
        if (t + 1 < plies && ((ply + 1) & 3u) == 0) block = draw_block(seed, env_base + (uint64_t)L.b, ply + 1);
        if (first_actions && t == 0) y = play_ply(p, row, mover, legal, action, illegal_mode);
        else y = play_ply<true>(p, row, mover, legal, action, illegal_mode);  // (sampled: legal by construction)
        dn = y.terminal ? 1 : 0;
        if (y.terminal) {  // raw_env.reset, gobblet.py:275-290
            p = Planes{0u, 0u, 0u};
            mover = 0;
            row.reset();
        }
        tcount = next_turn(tcount, y, 1);
        treset = treset || y.terminal;
        if (counters) {
            games += __popcll(__ballot(L.valid && y.terminal));
            w1 += __popcll(__ballot(L.valid && y.winner == 1));
            w2 += __popcll(__ballot(L.valid && y.winner == -1));
        }
        legal = legal54(p, mover);  // the next mover's: stored now, sampled from next ply
        if (t) pair_barrier();      // the images of the previous ply have been taken
        s_small[L.lane][0] = (uint32_t)action;
        s_small[L.lane][1] = ((uint32_t)y.winner & 0xFFu) | (((uint32_t)y.r0 & 0xFFu) << 8) | (((uint32_t)y.r1 & 0xFFu) << 16) |
                             ((uint32_t)dn << 24) | ((uint32_t)mover << 25);
        if (WITH_OBS) obs_scatter(s_obs, L.lane, p, mover);  // (into the zeroed image)
        if (WITH_MASK) mask_to_image<true>(s_mask, L.lane, legal);
        pair_barrier();  // images ready
    }
    pair_barrier();  // (the last ply's images taken: pairs with the storing wavefront's second barrier)
    wave_lds_fence();
    tile_out<kCells>(state + L.tile * (kTile * kCells), s_state, L.lane, L.rows);
    if (L.valid) {
        to_move[L.b] = (int8_t)mover;
        done[L.b] = (int8_t)dn;
        if (turn) turn[L.b] = treset ? tcount : turn[L.b] + tcount;
    }
    if (counters && L.lane == 0) tally_flush(counters, L.tile, L.rows, plies, games, w1, w2);
}

// gbl_collect for batches that do NOT fill the chip: ROLE wavefronts that share NOTHING, and the game played REDUNDANTLY wherever
// that saves a hand-over.  At 4 096 boards k_collect2's 64 workgroups leave three CUs in four idle and a ply lasts as long as
// its playing wavefront's serial path; a lone wavefront issues one instruction per 5-7 cycles whatever it is, so what counts is
// the number of instructions ONE wavefront executes per ply.  The game itself -- sample, move, winner, auto-reset, next legal
// mask: the CHAIN, ~250 instructions, every one depending on the ply before -- cannot be dealt out (0.72 us per ply with nothing
// stored, scripts/experiments/ab_floor.sh); everything else can.  A role wavefront loads a SUB-TILE of 64 / LPB boards (LPB lanes per board,
// all playing alike), plays every ply, and materialises one share of the outputs, 1 / LPB of a row per lane --
//   scalars: the five scalars of a ply, the tallies, and at the end the state (the only role that patches a state image);
//   mask:    the mask rows (lane j: bytes [64 j / LPB, 64 (j + 1) / LPB) of its board's row);
//   obs:     the observation rows (lane j: channels j, j + LPB, ...).
// No LDS hand-over, no cross-lane instruction; the redundant arithmetic runs on SIMDs that would idle.  A role's image of ply t
// is read back into registers at the end of its iteration and stored in the NEXT one, behind the sample and the move: the LDS
// round trip is off the chain.  Bit for bit the trajectories of k_collect (same sampler keys, same arithmetic).
//
// What a role costs a lone wavefront per ply (round 5, scripts/experiments/ab_roles.sh): the chain 0.72 us, + scalars ~0.05, + mask rows ~0.10
// whatever LPB, + observation rows 0.15 / 0.30 / 0.58 at 16 / 32 / 64 boards per wavefront: the observation role is the long one,
// and it alone gains from more lanes per board.  So a WORKGROUP is a group of 64 / LA boards with
//   one scalars wavefront (which also builds the mask rows when MERGE) and, unless MERGE, one mask wavefront, LA lanes per board,
//   KO observation wavefronts of LA * KO lanes per board, each over 1 / KO of the group,
// <LA, KO, MERGE> chosen by the batch size (collect_variant): every redundant chain is SIMD time that saturated SIMDs do not have.
// cell of sub-tile s (LPB lanes per board) at ply t: t * ply_stride + (s / LPB) * tile_stride + (s % LPB) * (64 / LPB).
// ONE barrier per launch (not per ply): the roles read the group's state, movers and first actions on their own and the scalars
// role overwrites them at the end -- the rendezvous behind the loads keeps a late role from reading what an early one wrote back
// (with one ply per launch the scalars role reaches its write-back after ~300 instructions).
constexpr int kRoleScalars = 1, kRoleMask = 2, kRoleObs = 4;  // (bits: a wavefront may hold several roles)

struct SmallArgs {
    int8_t *state, *to_move, *done;
    int64_t n;
    uint64_t seed, env_base;
    uint32_t ply0, plies;
    int64_t ply_stride, tile_stride;
    int32_t *actions_t;
    int8_t *winner_t, *reward_t, *done_t, *to_move_t, *mask_t, *obs_t;
    int illegal_mode;
    int64_t *counters;
    int32_t *turn;
    const int32_t *first_actions;
    int8_t *first_status;
};

template <int ROLE, int LPB, bool SYNC>
__device__ __forceinline__ void small_role(const SmallArgs &A, uint32_t *img, uint32_t *mask_img, uint32_t *obs_img, uint32_t *draw_buf,
                                           int64_t sub)
{
    constexpr int BPS = kTile / LPB, SH = LPB == 4 ? 2 : LPB == 2 ? 1 : 0;
    constexpr bool SC = (ROLE & kRoleScalars) != 0, MK = (ROLE & kRoleMask) != 0, OB = (ROLE & kRoleObs) != 0;
    const int lane = (int)(threadIdx.x & 63u), bq = lane >> SH, j = lane & (LPB - 1);
    const int64_t left = A.n - sub * BPS;
    if (left <= 0) {  // (an observation wavefront whose share of a ragged last group is empty: it still meets the others once)
#ifndef GBL_HOST_EMU
        if (SYNC) __syncthreads();
#endif
        return;
    }
    const int rows = left < BPS ? (int)left : BPS;
    const bool valid = bq < rows, full = rows == BPS;
    const int64_t b = sub * BPS + bq, bs = valid ? b : A.n - 1;
    int mover = A.to_move[bs];
    int given = A.first_actions ? A.first_actions[bs] : 0;  // (gbl_collect_from: the first ply plays the caller's actions)
    // The sampler's words.  One lane per board: a generator block per four plies, in registers, as k_collect.  LPB lanes per board:
    // the generator leaves the ply's serial chain -- lane j of a board generates block (base + j), the words of 4 LPB plies go
    // through LDS (16 bytes per lane), and a ply reads its word back one ply ahead: ~5 instead of ~30 instructions per ply.
    Draw4 block{{0u, 0u, 0u, 0u}};
    uint32_t base = A.ply0 >> 2;                            // the first generator block in draw_buf (wave-uniform)
    const uint32_t *const my_draws = draw_buf + (lane & ~(LPB - 1)) * 4;
    auto refill = [&](uint32_t blk) {                       // blocks blk .. blk + LPB - 1 of this wavefront's boards -> draw_buf
        const Draw4 d = draw_block(A.seed, A.env_base + (uint64_t)b, (blk + (uint32_t)j) << 2);
        reinterpret_cast<uint4 *>(draw_buf)[lane] = uint4{d.w[0], d.w[1], d.w[2], d.w[3]};
    };
    sub_in<kCells, BPS>(A.state + sub * (BPS * kCells), img, lane, rows, [&] {
        if constexpr (LPB == 1) block = draw_block(A.seed, A.env_base + (uint64_t)b, A.ply0);
        else refill(base);
    });
    wave_lds_fence();
    uint32_t r[7];
    row_load<kCells>(img, bq, r);
    r[6] &= 0x00FFFFFFu;
    uint32_t word = 0;                                      // the current ply's 32 random bits
    if constexpr (LPB > 1) word = my_draws[A.ply0 & 3u];
    if (SYNC) {
#ifndef GBL_HOST_EMU
        // every role's loads of the group have landed before the scalars role may write anything back (waits vmcnt(0) + lgkmcnt(0))
        asm volatile("" : "+v"(mover), "+v"(given));
        __syncthreads();
#endif
    }
    mover = valid && mover != 0;
    Planes p = make_planes(r);
    p.nz = valid ? p.nz : 0u;
    const ImageRow row{reinterpret_cast<uint8_t *>(img) + bq * kCells};
    uint32_t games = 0, w1 = 0, w2 = 0;
    Ply y{0, 0, 0, false, false};
    int dn = 0, tcount = 0;
    bool treset = false;
    uint64_t legal = legal54(p, mover);
    if (SC && A.first_status && valid && j == 0) A.first_status[b] = (int8_t)action_status_of(legal, given);  // (gbl_collect_from_ex)
    constexpr int kRowPolicy = kStoreStreamDrop;  // trajectory slots are written once: streamed
    // the images of the previous ply, on their way out
    SubVecs<MK ? sub_vectors<kActions, BPS>() : 0> vm{};
    SubVecs<OB ? sub_vectors<kObs, BPS>() : 0> vo{};
    int8_t *mdst = nullptr, *odst = nullptr;
    const int obytes = rows * kObs, mbytes = rows * kActions;  // what leaves of this sub-tile's images per ply
    const uint32_t plies = A.plies;
    const int64_t cell0 = (sub >> SH) * A.tile_stride + (sub & (LPB - 1)) * BPS;
    // this ply's rows of the two row streams: advanced by a ply's stride per ply (no 64-bit multiply inside the chain)
    int8_t *obs_at = OB ? A.obs_t + cell0 * kObs : nullptr, *mask_at = MK ? A.mask_t + cell0 * kActions : nullptr;
    const int64_t obs_step = A.ply_stride * kObs, mask_step = A.ply_stride * kActions;
    int64_t at = 0;  // ... and this ply's cell of the scalar arrays, relative to ply 0's (sc_* below)
    constexpr bool PAIR = LPB > 1;  // the lanes of a board split the winner test (winner_of_pair)
    // The scalars role's per-lane output arrays (NULL: this lane stores nothing there), at ply 0's cell of its board:
    //   4 lanes per board: lane 0 action + next mover, 1 reward, 2 winner, 3 done  (one byte store serves three arrays)
    //   2 lanes:           lane 0 action + next mover + winner, 1 reward + done
    //   1 lane:            everything
    int32_t *sc_act = nullptr;
    uint16_t *sc_rw = nullptr;
    int8_t *sc_b0 = nullptr, *sc_b1 = nullptr, *sc_b2 = nullptr;
    bool b0_is_mover = false, b0_is_winner = false;
    if (SC && valid) {
        const int64_t at0 = cell0 + bq;
        if (j == 0 && A.actions_t) sc_act = A.actions_t + at0;
        if (j == (LPB > 1 ? 1 : 0) && A.reward_t) sc_rw = reinterpret_cast<uint16_t *>(A.reward_t) + at0;
        if constexpr (LPB == 4) {
            b0_is_mover = j == 0;
            b0_is_winner = j == 2;
            int8_t *const arr = j == 0 ? A.to_move_t : j == 2 ? A.winner_t : j == 3 ? A.done_t : nullptr;
            if (arr) sc_b0 = arr + at0;
        } else if constexpr (LPB == 2) {
            b0_is_mover = j == 0;
            int8_t *const arr = j == 0 ? A.to_move_t : A.done_t;
            if (arr) sc_b0 = arr + at0;
            if (j == 0 && A.winner_t) sc_b1 = A.winner_t + at0;
        } else {
            if (A.winner_t) sc_b0 = A.winner_t + at0;
            if (A.done_t) sc_b1 = A.done_t + at0;
            if (A.to_move_t) sc_b2 = A.to_move_t + at0;
        }
    }
    GBL_PHASE_DECL;
    for (uint32_t t = 0; t < plies; ++t) {
        const uint32_t ply = A.ply0 + t;
        GBL_PHASE(0);  // loop overhead, the previous ply's tail
        if constexpr (LPB == 1) word = draw_word(block, ply);
        int action = pick54(legal, word);
        GBL_PHASE_DEP(1, action);  // the pick
        if (t + 1 < plies) {  // the next ply's word (nothing here depends on the game)
            if constexpr (LPB == 1) {
                if (((ply + 1) & 3u) == 0) block = draw_block(A.seed, A.env_base + (uint64_t)b, ply + 1);
            } else {
                uint32_t rel = ply + 1 - 4u * base;
                if (rel == 4u * LPB) {
                    wave_lds_fence();  // (every lane has taken this ply's word)
                    base += LPB;
                    refill(base);
                    wave_lds_fence();
                    rel = 0;
                }
                word = my_draws[rel];
            }
        }
        // (a sampled action is legal by construction: only the caller's actions of gbl_collect_from's first ply are tested)
        if (A.first_actions && t == 0) {
            action = given;
            if (SC)
                y = play_ply<false, PAIR>(p, row, mover, legal, action, A.illegal_mode, j);
            else
                y = play_ply<false, PAIR>(p, NoRow{}, mover, legal, action, A.illegal_mode, j);
        } else {
            if (SC)
                y = play_ply<true, PAIR>(p, row, mover, legal, action, A.illegal_mode, j);
            else
                y = play_ply<true, PAIR>(p, NoRow{}, mover, legal, action, A.illegal_mode, j);
        }
        GBL_PHASE_DEP(2, (uint32_t)y.winner + p.nz);  // the next word, move, winner
        dn = y.terminal ? 1 : 0;
        // the next mover's legal mask, of the moved position: it does not wait for the winner test (the two interleave on the lone
        // wavefront); a reset swaps in the empty board's
        uint64_t legal_next = legal54(p, mover);
        if (y.terminal) {  // raw_env.reset, gobblet.py:275-290
            p = Planes{0u, 0u, 0u};
            mover = 0;
            legal_next = kLegalEmpty;
            if (SC) row.reset();
        }
        GBL_PHASE_DEP(3, p.nz);  // reset
        if (t) {  // ply t - 1's rows (a ragged sub-tile's: the whole vectors of its rows)
            if constexpr (OB) sub_store<kObs, kRowPolicy, BPS>(odst, vo, lane, obytes & ~15);
            if constexpr (MK) sub_store<kActions, kRowPolicy, BPS>(mdst, vm, lane, mbytes & ~15);
        }
        if constexpr (SC) {
            tcount = next_turn(tcount, y, 1);
            treset = treset || y.terminal;
            if (A.counters) {  // (one lane per board counts)
                games += __popcll(__ballot(valid && j == 0 && y.terminal));
                w1 += __popcll(__ballot(valid && j == 0 && y.winner == 1));
                w2 += __popcll(__ballot(valid && j == 0 && y.winner == -1));
            }
            // the five scalars of a board, dealt over its lanes: per-lane array pointers fixed before the loop (sc_*), no branch
            // on the lane's index inside it
            {
                const uint16_t rw = (uint16_t)((y.r0 & 0xFF) | ((y.r1 & 0xFF) << 8));
                if (sc_act) sc_act[at] = action;
                if (sc_rw) sc_rw[at] = rw;
                if (sc_b0) sc_b0[at] = (int8_t)(LPB == 1 ? y.winner : b0_is_mover ? mover : b0_is_winner ? y.winner : dn);
                if constexpr (LPB <= 2) {
                    if (sc_b1) sc_b1[at] = (int8_t)(LPB == 1 ? dn : y.winner);
                }
                if constexpr (LPB == 1) {
                    if (sc_b2) sc_b2[at] = (int8_t)mover;
                }
                at += A.ply_stride;
            }
        }
        GBL_PHASE(4);  // the previous ply's row stores, this ply's scalars
        if constexpr (OB) {
            sub_obs_zero<BPS>(obs_img, lane);
            wave_lds_fence();
            obs_scatter_part<LPB>(reinterpret_cast<uint8_t *>(obs_img) + bq * kObs, p, mover, j);
            wave_lds_fence();
            odst = obs_at;
            obs_at += obs_step;
            sub_fetch<kObs, BPS>(obs_img, lane, vo);
            if (!full) sub_tail(odst, obs_img, lane, obytes);
            wave_lds_fence();
        }
        GBL_PHASE(5);  // the observation image
        legal = legal_next;  // stored now, sampled from next ply
        GBL_PHASE_DEP(6, (uint32_t)legal);  // the next legal mask
        if constexpr (MK) {
            mask_row_part<LPB>(reinterpret_cast<uint8_t *>(mask_img) + bq * kActions, legal, j);
            wave_lds_fence();
            mdst = mask_at;
            mask_at += mask_step;
            sub_fetch<kActions, BPS>(mask_img, lane, vm);
            if (!full) sub_tail(mdst, mask_img, lane, mbytes);
            wave_lds_fence();
        }
        GBL_PHASE(7);  // the mask image
    }
    GBL_PHASE(7);  // (the last ply's mask image; phase 7 = the mask image of every ply but the last, see below)
    GBL_PHASE_FLUSH(wave_index());
    if (plies) {  // the last ply's rows
        if constexpr (OB) sub_store<kObs, kRowPolicy, BPS>(odst, vo, lane, obytes & ~15);
        if constexpr (MK) sub_store<kActions, kRowPolicy, BPS>(mdst, vm, lane, mbytes & ~15);
    }
    if constexpr (SC) {
        wave_lds_fence();  // every board's byte patches are in the state image
        sub_out<kCells, kStorePlain, BPS>(A.state + sub * (BPS * kCells), img, lane, rows);
        if (valid && j == 0) {
            A.to_move[b] = (int8_t)mover;
            A.done[b] = (int8_t)dn;
            if (A.turn) A.turn[b] = treset ? tcount : A.turn[b] + tcount;
        }
        if (A.counters && lane == 0) tally_flush(A.counters, sub >> SH, rows, plies, games, w1, w2);
    }
}

// gbl_collect between the role kernel and the HBM-bound regime: k_collect3 -- ONE wavefront plays a tile's game, and hands every
// ply's position (planes, mover, next legal mask: six dwords per board, double-buffered in LDS, ONE barrier per ply) to a mask-row
// wavefront and an observation-row wavefront, which build, read back and store their rows.  Against k_collect2 (one wavefront
// plays AND builds both images, one takes them over and stores: two barriers per ply, ~360 against ~60 instructions per ply) the
// work is dealt evenly -- player ~235 (chain + scalars), mask ~80, observation ~200 -- and nothing is played twice, so it keeps
// paying where the role kernel's redundant chains run out of idle SIMDs (from ~32 768 boards, three wavefronts per tile and SIMD).
// Bit for bit the trajectories of k_collect.
// HAND: the first row wavefront stores the ply's five scalars, which ride over with the legal mask -- ~25 instructions off the playing
// wavefront, whose chain the launch waits for (MASK_ONLY 12 288 boards 0.63 -> 0.56 us per ply, 32 768: 0.67 -> 0.61, 262 144: 3.02 -> 2.75,
// 524 288: 5.6 -> 5.2; FULL 20 480 ... 45 056: -2 ... -3 %).  Not beyond 524 288 boards: there MASK_ONLY runs at the chip's write rate on
// every wavefront it can get, and the 1 KB of LDS the wider hand-over costs a workgroup is 3 % (786 432 boards 7.48 -> 7.72, 2^20:
// 9.81 -> 10.07 whoever stores the scalars; profiles/r05/ab_trio_scalars.txt).
template <bool WITH_MASK, bool WITH_OBS, bool DEV_PLY, bool HAND>
__global__ __launch_bounds__(64 * (1 + (WITH_MASK ? 1 : 0) + (WITH_OBS ? 1 : 0))) void k_collect3(
    int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n, int64_t ntiles, uint64_t seed, uint64_t env_base,
    const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies, int8_t *__restrict__ done, int64_t ply_stride,
    int64_t tile_stride, int32_t *__restrict__ actions_t, int8_t *__restrict__ winner_t, int8_t *__restrict__ reward_t,
    int8_t *__restrict__ done_t, int8_t *__restrict__ to_move_t, int8_t *__restrict__ mask_t, int8_t *__restrict__ obs_t,
    int illegal_mode, int64_t *__restrict__ counters, int32_t *__restrict__ turn, const int32_t *__restrict__ first_actions,
    int8_t *__restrict__ first_status)
{
    constexpr int WAVES = 1 + (WITH_MASK ? 1 : 0) + (WITH_OBS ? 1 : 0);
    __shared__ uint32_t s_state[image_words<kCells>()];
    __shared__ uint32_t s_obs[WITH_OBS ? image_words<kObs>() : 4];
    __shared__ uint32_t s_mask[WITH_MASK ? image_words<kActions>() : 4];
    __shared__ uint4 s_hand[2][kTile];      // per ply parity and board: nz, neg, odd, mover
    // ... the next mover's legal mask (x, y) and, HAND, the ply's scalars for the first row wavefront to store: z = the action played,
    // w = winner | r0 << 8 | r1 << 16 | done << 24 | next mover << 25
    using LegalSlot = typename std::conditional<HAND, uint4, uint2>::type;
    __shared__ LegalSlot s_legal[2][kTile];
    if (DEV_PLY) ply0 += *ply_dev;
    const int role = WAVES > 1 ? wave_index() : 0;
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t tile = (int64_t)blockIdx.x;
    if (tile >= ntiles) return;  // (the same for every wavefront of the workgroup)
    const int64_t left = n - tile * kTile;
    const int rows = left < kTile ? (int)left : kTile;
    const bool valid = lane < rows, full = rows == kTile;
    const int64_t b = tile * kTile + lane;
    constexpr int kPolicy = kStoreStreamDrop;
    const int64_t cell0 = tile * tile_stride;
    constexpr bool hand_scalars = HAND && WAVES > 1;  // (a launch without mask and observation arrays has nobody to hand them to)
    if (role != 0) {
        // ---- a row wavefront: the mask rows (role 1 when there are any) or the observation rows -----------------------------
        const bool is_mask = WITH_MASK && role == 1;
        SubVecs<WITH_MASK ? sub_vectors<kActions, kTile>() : 0> vm{};
        SubVecs<WITH_OBS ? sub_vectors<kObs, kTile>() : 0> vo{};
        int8_t *dst = nullptr;
        // this ply's rows: advanced by a ply's stride per ply (no 64-bit multiply per ply)
        int8_t *row_at = is_mask ? mask_t + cell0 * kActions : obs_t + cell0 * kObs;
        const int64_t row_step = ply_stride * (is_mask ? kActions : kObs);
        int64_t scell = cell0 + lane;  // (role 1) this lane's cell of the scalar arrays at ply t
        for (uint32_t t = 0; t < plies; ++t) {
            pair_barrier();  // ply t's positions are in s_hand[t & 1] (and the player is free to go on with ply t + 1)
            if constexpr (hand_scalars) {
                if (role == 1) {  // the ply's five scalars leave from here
                    const uint4 sc = s_legal[t & 1u][lane];
                    if (valid) {
                        if (actions_t) actions_t[scell] = (int32_t)sc.z;
                        if (winner_t) winner_t[scell] = (int8_t)(sc.w & 0xFFu);
                        if (reward_t) reinterpret_cast<uint16_t *>(reward_t)[scell] = (uint16_t)((sc.w >> 8) & 0xFFFFu);
                        if (done_t) done_t[scell] = (int8_t)((sc.w >> 24) & 1u);
                        if (to_move_t) to_move_t[scell] = (int8_t)((sc.w >> 25) & 1u);
                    }
                    scell += ply_stride;
                }
            }
            if (t) {  // ply t - 1's rows, read back at the end of the last iteration (a ragged tile's: the whole vectors of its rows)
                if constexpr (WITH_MASK) {
                    if (is_mask) sub_store<kActions, kPolicy, kTile>(dst, vm, lane, (rows * kActions) & ~15);
                }
                if constexpr (WITH_OBS) {
                    if (!is_mask) sub_store<kObs, kPolicy, kTile>(dst, vo, lane, (rows * kObs) & ~15);
                }
            }
            if constexpr (WITH_MASK) {
                if (is_mask) {
                    const LegalSlot lg = s_legal[t & 1u][lane];
                    mask_row_part<1>(reinterpret_cast<uint8_t *>(s_mask) + lane * kActions, ((uint64_t)lg.y << 32) | lg.x, 0);
                    wave_lds_fence();
                    dst = row_at;
                    sub_fetch<kActions, kTile>(s_mask, lane, vm);
                    if (!full) sub_tail(dst, s_mask, lane, rows * kActions);
                    wave_lds_fence();
                }
            }
            if constexpr (WITH_OBS) {
                if (!is_mask) {
                    const uint4 h = s_hand[t & 1u][lane];
                    sub_obs_zero<kTile>(s_obs, lane);
                    wave_lds_fence();
                    obs_scatter_row(reinterpret_cast<uint8_t *>(s_obs) + lane * kObs, Planes{h.x, h.y, h.z}, (int)h.w);
                    wave_lds_fence();
                    dst = row_at;
                    sub_fetch<kObs, kTile>(s_obs, lane, vo);
                    if (!full) sub_tail(dst, s_obs, lane, rows * kObs);
                    wave_lds_fence();
                }
            }
            row_at += row_step;
        }
        if (plies) {  // the last ply's rows
            if constexpr (WITH_MASK) {
                if (is_mask) sub_store<kActions, kPolicy, kTile>(dst, vm, lane, (rows * kActions) & ~15);
            }
            if constexpr (WITH_OBS) {
                if (!is_mask) sub_store<kObs, kPolicy, kTile>(dst, vo, lane, (rows * kObs) & ~15);
            }
        }
        return;
    }
    // ---- the playing wavefront: k_collect's loop with the scalars, without the rows -----------------------------------------
    // (s_setprio 3 on the player, so that it wins the issue arbitration against the row wavefronts of its SIMD: no effect at any size,
    //  profiles/r05/player_prio.txt)
    Lane L;
    L.tile = tile; L.lane = lane; L.rows = rows; L.valid = valid; L.b = b;
    int mover = to_move[valid ? b : n - 1];
    int given = first_actions ? first_actions[valid ? b : n - 1] : 0;  // (gbl_collect_from, see k_collect)
    uint32_t r[7];
    Draw4 block{{0u, 0u, 0u, 0u}};
    load_state(state, s_state, L, r, [&] { block = draw_block(seed, env_base + (uint64_t)b, ply0); });
    mover = valid && mover != 0;
    Planes p = planes_of(L, r);
    const ImageRow row{reinterpret_cast<uint8_t *>(s_state) + lane * kCells};
    uint32_t games = 0, w1 = 0, w2 = 0;
    Ply y{0, 0, 0, false, false};
    int dn = 0, tcount = 0;
    bool treset = false;
    uint64_t legal = legal54(p, mover);
    if (first_status && valid) first_status[b] = (int8_t)action_status_of(legal, given);  // (gbl_collect_from_ex)
    int64_t cell = cell0;  // ply t's cell of the tile in the scalar arrays
    for (uint32_t t = 0; t < plies; ++t) {
        const uint32_t ply = ply0 + t;
        int action = pick54(legal, draw_word(block, ply));
        if (t + 1 < plies && ((ply + 1) & 3u) == 0) block = draw_block(seed, env_base + (uint64_t)b, ply + 1);
        if (first_actions && t == 0) {
            action = given;
            y = play_ply(p, row, mover, legal, action, illegal_mode);
        } else {
            y = play_ply<true>(p, row, mover, legal, action, illegal_mode);  // (sampled: legal by construction)
        }
        dn = y.terminal ? 1 : 0;
        legal = legal54(p, mover);  // the next mover's (beside the winner test, see small_role): stored now, sampled from next ply
        if (y.terminal) {  // raw_env.reset, gobblet.py:275-290
            p = Planes{0u, 0u, 0u};
            mover = 0;
            legal = kLegalEmpty;
            row.reset();
        }
        s_hand[t & 1u][lane] = uint4{p.nz, p.neg, p.odd, (uint32_t)mover};
        if constexpr (HAND)
            s_legal[t & 1u][lane] = uint4{(uint32_t)legal, (uint32_t)(legal >> 32), (uint32_t)action,
                                          ((uint32_t)y.winner & 0xFFu) | (((uint32_t)y.r0 & 0xFFu) << 8) | (((uint32_t)y.r1 & 0xFFu) << 16) |
                                              ((uint32_t)dn << 24) | ((uint32_t)mover << 25)};
        else
            s_legal[t & 1u][lane] = uint2{(uint32_t)legal, (uint32_t)(legal >> 32)};
        if (WAVES > 1) pair_barrier();  // ply t handed over
        tcount = next_turn(tcount, y, 1);
        treset = treset || y.terminal;
        if (counters) {
            games += __popcll(__ballot(valid && y.terminal));
            w1 += __popcll(__ballot(valid && y.winner == 1));
            w2 += __popcll(__ballot(valid && y.winner == -1));
        }
        if (!hand_scalars && valid) {
            const int64_t at = cell + lane;
            if (actions_t) actions_t[at] = action;
            if (winner_t) winner_t[at] = (int8_t)y.winner;
            if (reward_t) reinterpret_cast<uint16_t *>(reward_t)[at] = (uint16_t)((y.r0 & 0xFF) | ((y.r1 & 0xFF) << 8));
            if (done_t) done_t[at] = (int8_t)dn;
            if (to_move_t) to_move_t[at] = (int8_t)mover;
        }
        cell += ply_stride;
    }
    wave_lds_fence();
    tile_out<kCells>(state + tile * (kTile * kCells), s_state, lane, rows);
    if (valid) {
        to_move[b] = (int8_t)mover;
        done[b] = (int8_t)dn;
        if (turn) turn[b] = treset ? tcount : turn[b] + tcount;
    }
    if (counters && lane == 0) tally_flush(counters, tile, rows, plies, games, w1, w2);
}

// wavefronts of a workgroup of the role kernel: the scalars wavefront, the mask wavefront unless merged, KO observation wavefronts
// (KO = 0, MERGE: ONE wavefront per group holds all three roles -- A/B builds only, see scripts/experiments/ab_oneply.py)
template <bool WITH_MASK, bool WITH_OBS, int KO, bool MERGE>
constexpr int small_waves() { return 1 + ((WITH_MASK && !MERGE) ? 1 : 0) + (WITH_OBS ? KO : 0); }

// (The one-ply entry points -- gbl_rollout with plies = 1, gbl_step -- were routed here too and gained nothing: 3.34-3.47 us per
// launch against k_rollout's 3.29-3.36 at 1 024 - 4 096 boards, scripts/experiments/ab_ply.sh: a one-ply launch is its tile load, the chain
// and the launch boundary, none of which a smaller tile shortens.  They stay on k_rollout / k_step.)
template <bool WITH_MASK, bool WITH_OBS, bool DEV_PLY, int LA, int KO, bool MERGE>
__global__ __launch_bounds__((64 * small_waves<WITH_MASK, WITH_OBS, KO, MERGE>())) void k_collect_small(
    int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n, int64_t ngroups, uint64_t seed, uint64_t env_base,
    const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies, int8_t *__restrict__ done, int64_t ply_stride,
    int64_t tile_stride, int32_t *__restrict__ actions_t, int8_t *__restrict__ winner_t, int8_t *__restrict__ reward_t,
    int8_t *__restrict__ done_t, int8_t *__restrict__ to_move_t, int8_t *__restrict__ mask_t, int8_t *__restrict__ obs_t,
    int illegal_mode, int64_t *__restrict__ counters, int32_t *__restrict__ turn, const int32_t *__restrict__ first_actions,
    int8_t *__restrict__ first_status)
{
    static_assert(LA * KO <= 4 && (KO > 0 || MERGE), "at most four lanes per board");
    constexpr int WAVES = small_waves<WITH_MASK, WITH_OBS, KO, MERGE>(), NA = WAVES - (WITH_OBS ? KO : 0);
    constexpr int GB = kTile / LA, LO = LA * (KO ? KO : 1), OBB = kTile / LO;  // boards per group; observation wavefronts: LO lanes per board, OBB boards
    constexpr int kStateWords = GB * kCells / 4 + 4, kObsWords = OBB * kObs / 4 + 4, kMaskWords = GB * kActions / 4 + 4;
    __shared__ uint32_t s_state[WAVES][kStateWords];
    __shared__ uint32_t s_obs[WITH_OBS && KO ? KO : 1][WITH_OBS ? kObsWords : 4];
    __shared__ uint32_t s_mask[WITH_MASK ? kMaskWords : 4];
    __shared__ uint4 s_draw[LO > 1 ? WAVES : 1][LO > 1 ? 64 : 1];  // the sampler's words of 4 LPB plies, 16 bytes per lane
    if (DEV_PLY) ply0 += *ply_dev;
    const int64_t group = (int64_t)blockIdx.x;
    if (group >= ngroups) return;
    const int wave = WAVES > 1 ? wave_index() : 0;
    const SmallArgs A{state, to_move, done, n, seed, env_base, ply0, plies, ply_stride, tile_stride, actions_t, winner_t, reward_t,
                      done_t, to_move_t, mask_t, obs_t, illegal_mode, counters, turn, first_actions, first_status};
    constexpr bool SYNC = WAVES > 1;
    if (wave == 0) {
        small_role<kRoleScalars | ((WITH_MASK && MERGE) ? kRoleMask : 0) | ((WITH_OBS && KO == 0) ? kRoleObs : 0), LA, SYNC>(
            A, s_state[0], s_mask, s_obs[0], reinterpret_cast<uint32_t *>(s_draw[0]), group);
        return;
    }
    if constexpr (WITH_MASK && !MERGE) {
        if (wave == 1) {
            small_role<kRoleMask, LA, SYNC>(A, s_state[1], s_mask, nullptr, reinterpret_cast<uint32_t *>(s_draw[LO > 1 ? 1 : 0]), group);
            return;
        }
    }
    if constexpr (WITH_OBS && KO > 0)
        small_role<kRoleObs, LO, SYNC>(A, s_state[wave], nullptr, s_obs[wave - NA], reinterpret_cast<uint32_t *>(s_draw[LO > 1 ? wave : 0]),
                                       group * KO + (wave - NA));
}

// gbl_collect for batches that do not fill the chip, round 6: the role kernel's GEOMETRY -- groups of 32 boards, four wavefronts, each
// alone on a SIMD -- with k_collect3's HAND-OVER instead of redundant chains.  In the role kernel every role wavefront replays the
// whole game (150 instructions per ply) before it builds its share of the rows; here ONE wavefront plays a group -- two lanes per
// board, the winner test split over the pair -- and does nothing else: it leaves every ply's position, legal mask, action and results
// in an LDS ring of 2 x 4 plies and meets the row wavefronts once per four plies.  They take it from there:
//   wave 1   the mask rows (two lanes per board), the ply's five scalars dealt over the pair, the tallies and turn counters, and the
//            sampler's generator (one Philox block per board and group of four plies into a four-block ring, three ahead);
//   wave 2,3 the observation rows of 16 boards each, four lanes per board.
// The boards live in the player's planes for the whole launch; the 27-byte rows are rebuilt from them once, at the end
// (planes_to_row: bytes outside the state contract are not preserved).  Bit for bit the trajectories of k_collect.
constexpr int kGroupBoards = 32, kGroupRing = 4;

template <bool WITH_OBS, bool DEV_PLY>
__global__ __launch_bounds__(64 * (WITH_OBS ? 4 : 2)) void k_collect5(
    int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n, int64_t ngroups, uint64_t seed, uint64_t env_base,
    const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies, int8_t *__restrict__ done, int64_t ply_stride,
    int64_t tile_stride, int32_t *__restrict__ actions_t, int8_t *__restrict__ winner_t, int8_t *__restrict__ reward_t,
    int8_t *__restrict__ done_t, int8_t *__restrict__ to_move_t, int8_t *__restrict__ mask_t, int8_t *__restrict__ obs_t,
    int illegal_mode, int64_t *__restrict__ counters, int32_t *__restrict__ turn, const int32_t *__restrict__ first_actions,
    int8_t *__restrict__ first_status)
{
    constexpr int GB = kGroupBoards, OBB = 16;
    static_assert(kGroupRing == 4, "slot = t & 7, one generator block per group of plies");
    __shared__ uint32_t s_state[GB * kCells / 4 + 4];
    __shared__ uint32_t s_mask[GB * kActions / 4 + 4];
    __shared__ uint32_t s_obs[WITH_OBS ? 2 : 1][WITH_OBS ? OBB * kObs / 4 + 4 : 4];
    __shared__ uint4 s_hand[2 * kGroupRing][GB];   // per ply slot and board: nz, neg, odd, next mover
    __shared__ uint4 s_legal[2 * kGroupRing][GB];  // ... the next mover's legal mask (x, y), the action played (z), and in w: winner | r0 << 8 |
                                                   //     r1 << 16 | done << 24 | next mover << 25 | stepped << 26
    __shared__ uint4 s_draw[4][GB];                // the sampler's words: block m of board b (plies 4 m ... 4 m + 3) at [m & 3][b]
    if (DEV_PLY) ply0 += *ply_dev;
    const int role = wave_index();
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t group = (int64_t)blockIdx.x;
    if (group >= ngroups) return;  // (the same for every wavefront of the workgroup)
    const int64_t left = n - group * GB;
    const int rows = left < GB ? (int)left : GB;
    constexpr int kPolicy = kStoreStreamDrop;
    const int64_t cell0 = (group >> 1) * tile_stride + (group & 1) * GB;  // the group's first cell of ply 0 (a tile is two groups)
    const uint32_t m0 = ply0 >> 2;
    const uint32_t groups_of_plies = (plies + kGroupRing - 1) / kGroupRing;
    if (role == 1) {
        // ---- the mask rows, the scalars, the tallies, the turn counters, the generator: two lanes per board ----------------------
        const int bq = lane >> 1, j = lane & 1;
        const bool valid = bq < rows;
        const int64_t b = group * GB + bq;
        SubVecs<sub_vectors<kActions, GB>()> vm{};
        int8_t *dst = nullptr, *row_at = mask_t + cell0 * kActions;
        const int64_t row_step = ply_stride * kActions;
        const int mbytes = rows * kActions;
        // the five scalars of a board dealt over its pair (as the role kernel's scalars role): lane 0 action + next mover + winner,
        // lane 1 reward + done; per-lane array pointers fixed here, no branch on the lane's index inside the loop
        int32_t *sc_act = nullptr;
        uint16_t *sc_rw = nullptr;
        int8_t *sc_b0 = nullptr, *sc_b1 = nullptr;
        if (valid) {
            const int64_t at0 = cell0 + bq;
            if (j == 0 && actions_t) sc_act = actions_t + at0;
            if (j == 1 && reward_t) sc_rw = reinterpret_cast<uint16_t *>(reward_t) + at0;
            int8_t *const arr = j == 0 ? to_move_t : done_t;
            if (arr) sc_b0 = arr + at0;
            if (j == 0 && winner_t) sc_b1 = winner_t + at0;
        }
        int64_t at = 0;
        uint32_t games = 0, w1 = 0, w2 = 0;
        int tcount = 0;
        bool treset = false;
        auto generate = [&](uint32_t m) {
            const Draw4 d = draw_block(seed, env_base + (uint64_t)b, m << 2);
            s_draw[m & 3u][bq] = uint4{d.w[0], d.w[1], d.w[2], d.w[3]};  // (both lanes of a board: the same words)
        };
        generate(m0);
        generate(m0 + 1u);
        generate(m0 + 2u);
        pair_barrier();  // setup: the first draws are in LDS
        for (uint32_t g = 0; g < groups_of_plies; ++g) {
            pair_barrier();  // plies 4 g ... 4 g + 3 are in slots (g & 1) * 4 ... + 3 (and the player is free to play the next four)
            // the generator, three blocks ahead of this wavefront's own consumption: block m0 + g + 3 replaces block m0 + g - 1, which
            // the player (now in plies 4 g + 4 ...: blocks m0 + g + 1, m0 + g + 2) has left behind
            generate(m0 + g + 3u);
            const uint32_t t_end = (g + 1u) * kGroupRing < plies ? (g + 1u) * kGroupRing : plies;
#pragma nounroll
            for (uint32_t t = g * kGroupRing; t < t_end; ++t) {
                const uint4 sc = s_legal[t & (2u * kGroupRing - 1u)][bq];
                {
                    const uint32_t winner = sc.w & 0xFFu, dn = (sc.w >> 24) & 1u, mv = (sc.w >> 25) & 1u;
                    if (sc_act) sc_act[at] = (int32_t)sc.z;
                    if (sc_rw) sc_rw[at] = (uint16_t)((sc.w >> 8) & 0xFFFFu);
                    if (sc_b0) sc_b0[at] = (int8_t)(j == 0 ? mv : dn);
                    if (sc_b1) sc_b1[at] = (int8_t)winner;
                    at += ply_stride;
                    const bool terminal = dn != 0;
                    tcount = terminal ? 0 : tcount + (int)((sc.w >> 26) & 1u);  // raw_env.turn: + 1 per step, 0 after a reset (next_turn)
                    treset = treset || terminal;
                    if (counters) {  // (one lane per board counts)
                        const int w = (int)(int8_t)winner;
                        games += __popcll(__ballot(valid && j == 0 && terminal));
                        w1 += __popcll(__ballot(valid && j == 0 && w == 1));
                        w2 += __popcll(__ballot(valid && j == 0 && w == -1));
                    }
                }
                if (t) sub_store<kActions, kPolicy, GB>(dst, vm, lane, mbytes & ~15);  // ply t - 1's rows (a ragged group's: the whole vectors)
                mask_row_part<2>(reinterpret_cast<uint8_t *>(s_mask) + bq * kActions, ((uint64_t)sc.y << 32) | sc.x, j);
                wave_lds_fence();
                dst = row_at;
                row_at += row_step;
                sub_fetch<kActions, GB>(s_mask, lane, vm);
                if (rows != GB) sub_tail(dst, s_mask, lane, mbytes);
                wave_lds_fence();
            }
        }
        if (plies) sub_store<kActions, kPolicy, GB>(dst, vm, lane, mbytes & ~15);
        if (valid && j == 0 && turn) turn[b] = treset ? tcount : turn[b] + tcount;
        if (counters && lane == 0) tally_flush(counters, group >> 1, rows, plies, games, w1, w2);
        return;
    }
    if (role >= 2) {
        if constexpr (WITH_OBS) {
            // ---- the observation rows of 16 boards: four lanes per board -------------------------------------------------------
            const int ow = role - 2, oq = lane >> 2, oj = lane & 3;
            const int orows_all = rows - ow * OBB, orows = orows_all < 0 ? 0 : orows_all > OBB ? OBB : orows_all;
            const int obytes = orows * kObs;
            uint32_t *const img = s_obs[ow];
            SubVecs<sub_vectors<kObs, OBB>()> vo{};
            int8_t *dst = nullptr, *row_at = obs_t + (cell0 + ow * OBB) * kObs;
            const int64_t row_step = ply_stride * kObs;
            pair_barrier();  // setup
            for (uint32_t g = 0; g < groups_of_plies; ++g) {
                pair_barrier();
                const uint32_t t_end = (g + 1u) * kGroupRing < plies ? (g + 1u) * kGroupRing : plies;
#pragma nounroll
                for (uint32_t t = g * kGroupRing; t < t_end; ++t) {
                    const uint4 h = s_hand[t & (2u * kGroupRing - 1u)][ow * OBB + oq];
                    if (t) sub_store<kObs, kPolicy, OBB>(dst, vo, lane, obytes & ~15);
                    sub_obs_zero<OBB>(img, lane);
                    wave_lds_fence();
                    obs_scatter_part<4>(reinterpret_cast<uint8_t *>(img) + oq * kObs, Planes{h.x, h.y, h.z}, (int)h.w, oj);
                    wave_lds_fence();
                    dst = row_at;
                    row_at += row_step;
                    sub_fetch<kObs, OBB>(img, lane, vo);
                    if (orows != OBB) sub_tail(dst, img, lane, obytes);
                    wave_lds_fence();
                }
            }
            if (plies) sub_store<kObs, kPolicy, OBB>(dst, vo, lane, obytes & ~15);
        }
        return;
    }
    // ---- the playing wavefront: the game and the hand-over, nothing else; two lanes per board -----------------------------------
    const int bq = lane >> 1, j = lane & 1;
    const bool valid = bq < rows;
    const int64_t b = group * GB + bq, bs = valid ? b : n - 1;
    int mover = to_move[bs];
    int given = first_actions ? first_actions[bs] : 0;  // (gbl_collect_from, see k_collect)
    sub_in<kCells, GB>(state + group * (GB * kCells), s_state, lane, rows);
    wave_lds_fence();
    uint32_t r[7];
    row_load<kCells>(s_state, bq, r);
    r[6] &= 0x00FFFFFFu;
    mover = valid && mover != 0;
    Planes p = make_planes(r);
    p.nz = valid ? p.nz : 0u;
    int dn = 0;
    uint64_t legal = legal54(p, mover);
    if (first_status && valid && j == 0) first_status[b] = (int8_t)action_status_of(legal, given);  // (gbl_collect_from_ex)
    pair_barrier();  // setup: the first draws are in LDS
    const uint32_t *const my_draws = reinterpret_cast<const uint32_t *>(&s_draw[0][bq]);  // word w of block m: [(m & 3) * 4 GB + w]
    uint32_t word = my_draws[(m0 & 3u) * (GB * 4) + (ply0 & 3u)];
    for (uint32_t t = 0; t < plies; ++t) {
        int action = pick54(legal, word);
        {  // the next ply's word (its block was generated at least a group of plies ago): the LDS round trip hides behind this ply
            const uint32_t nx = ply0 + t + 1u;
            word = my_draws[((nx >> 2) & 3u) * (GB * 4) + (nx & 3u)];
        }
        Ply y;
        if (first_actions && t == 0) {
            action = given;
            y = play_ply<false, true>(p, NoRow{}, mover, legal, action, illegal_mode, j);
        } else {
            y = play_ply<true, true>(p, NoRow{}, mover, legal, action, illegal_mode, j);  // (sampled: legal by construction)
        }
        dn = y.terminal ? 1 : 0;
        legal = legal54(p, mover);  // the next mover's (beside the winner test, see small_role): stored now, sampled from next ply
        if (y.terminal) {  // raw_env.reset, gobblet.py:275-290
            p = Planes{0u, 0u, 0u};
            mover = 0;
            legal = kLegalEmpty;
        }
        const uint32_t slot = t & (2u * kGroupRing - 1u);
        s_hand[slot][bq] = uint4{p.nz, p.neg, p.odd, (uint32_t)mover};  // (both lanes of a board: the same values)
        s_legal[slot][bq] = uint4{(uint32_t)legal, (uint32_t)(legal >> 32), (uint32_t)action,
                                  ((uint32_t)y.winner & 0xFFu) | (((uint32_t)y.r0 & 0xFFu) << 8) | (((uint32_t)y.r1 & 0xFFu) << 16) |
                                      ((uint32_t)dn << 24) | ((uint32_t)mover << 25) | ((y.stepped ? 1u : 0u) << 26)};
        if ((t & (kGroupRing - 1u)) == kGroupRing - 1u || t + 1u == plies) pair_barrier();  // four plies handed over
    }
    // the boards as they stand, rebuilt from the planes; lane 0 of every pair leaves its row in the image (27-byte rows: unaligned
    // LDS stores, as ImageRow::reset), the image goes out as the load brought it in
    planes_to_row(p, r);
    wave_lds_fence();
    if (j == 0) __builtin_memcpy(reinterpret_cast<uint8_t *>(s_state) + bq * kCells, r, kCells);
    wave_lds_fence();
    sub_out<kCells, kStorePlain, GB>(state + group * (GB * kCells), s_state, lane, rows);
    if (valid && j == 0) {
        to_move[b] = (int8_t)mover;
        done[b] = (int8_t)dn;
    }
}

// gbl_placement_probe: the write pattern of k_collect without the game -- tile i of `plies` slots stores 64 rows of
// 117 bytes into a and 64 rows of 54 bytes into b (zeros, `nt sc1` like the trajectory stream), one wavefront per
// tile, identity tile map.  Timed with both streams, with a alone and with b alone (see the header).
template <bool WITH_A, bool WITH_B>
__global__ __launch_bounds__(64) void k_probe(int8_t *__restrict__ a, int8_t *__restrict__ b, int64_t ntiles, int plies)
{
    __shared__ uint32_t s_img[image_words<kObs>()];
    const int lane = threadIdx.x;
    const int64_t tile = blockIdx.x;
    if (tile >= ntiles) return;
    obs_image_zero(s_img, lane);
    wave_lds_fence();
    for (int t = 0; t < plies; ++t) {
        const int64_t cell = ((int64_t)t * ntiles + tile) * kTile;
        if (WITH_A) tile_out<kObs, kStoreStreamDrop>(a + cell * kObs, s_img, lane, kTile);
        if (WITH_B) tile_out<kActions, kStoreStreamDrop>(b + cell * kActions, s_img, lane, kTile);
    }
}

// gbl_counter_add: the device-resident ply / call counter of the *_at entry points
__global__ void k_counter_add(uint32_t *ctr, uint32_t by) { *ctr += by; }

// gbl_sample: mask rows -> one action per board
__global__ __launch_bounds__(64) void k_sample(const int8_t *__restrict__ mask, int32_t *__restrict__ actions, int64_t n,
                                               int64_t ntiles, uint64_t seed, uint64_t env_base, uint32_t ply,
                                               const uint32_t *__restrict__ ply_dev)
{
    if (ply_dev) ply += *ply_dev;
    __shared__ uint32_t s_mask[image_words<kActions>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    uint32_t draw = 0;  // board-independent: computed while the tile is in flight
    tile_in<kActions>(mask + L.tile * (kTile * kActions), s_mask, L.lane, L.rows,
                      [&] { draw = draw32(seed, env_base + (uint64_t)L.b, ply); });
    wave_lds_fence();
    uint32_t d[14];
    row_load<kActions>(s_mask, L.lane, d);
    if (!L.valid) return;
    actions[L.b] = pick54(mask_bits(d), draw);
}

// gbl_decode_obs: greedy_policy.py:43-71
__global__ __launch_bounds__(64) void k_decode_obs(const int8_t *__restrict__ obs, int8_t *__restrict__ state,
                                                   int8_t *__restrict__ to_move, int64_t n, int64_t ntiles)
{
    __shared__ uint32_t s_obs[image_words<kObs>()];
    __shared__ uint32_t s_state[image_words<kCells>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    tile_in<kObs>(obs + L.tile * (kTile * kObs), s_obs, L.lane, L.rows);
    wave_lds_fence();
    uint32_t d[30];
    row_load<kObs>(s_obs, L.lane, d);
    uint32_t r[7];
    int agent = decode_obs_row(d, r);
    row_stage<kCells>(s_state, L.lane, r);
    wave_lds_fence();
    tile_out<kCells>(state + L.tile * (kTile * kCells), s_state, L.lane, L.rows);
    if (L.valid) to_move[L.b] = (int8_t)agent;
}

// gbl_validate: state-contract flags per board
__global__ __launch_bounds__(64) void k_validate(const int8_t *__restrict__ state, int8_t *__restrict__ flags, int64_t n,
                                                 int64_t ntiles)
{
    __shared__ uint32_t s_state[image_words<kCells>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    uint32_t r[7];
    load_state(state, s_state, L, r);
    if (!L.valid) return;
    flags[L.b] = (int8_t)validate_row(r);
}

// ---- the search kernels (k_playout, k_tree, k_collect_search): what they share ----------------------------------------------------
__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

// Butterfly reductions over the wavefront: every lane returns with the full result.
template <typename T>
__device__ __forceinline__ T wave_max(T x)  // (T: uint32_t, uint64_t or int32_t)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const T other = __shfl_xor(x, o);
        x = other > x ? other : x;
    }
    return x;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x)  // (a signed sum goes through a cast: two's complement, the same bits)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += (uint32_t)__shfl_xor((int)x, o);
    return x;
}

// Board b's planes in every lane: lane c < 27 reads cell c, and three ballots are the planes.
__device__ __forceinline__ Planes board_planes(const int8_t *__restrict__ state, int64_t b, uint32_t lane)
{
    const int v = lane < (uint32_t)kCells ? state[b * kCells + lane] : 0;
    return Planes{(uint32_t)__ballot(v != 0), (uint32_t)__ballot(v < 0), (uint32_t)__ballot(v & 1)};
}

// ... and the candidates of its search: the mover's legal actions, less those whose byte of the board's `mask` row (optional) is zero
__device__ __forceinline__ uint64_t board_candidates(const Planes &p, int mover, const int8_t *__restrict__ mask, int64_t b, uint32_t lane)
{
    uint64_t cand = legal54(p, mover);
    if (mask) cand &= (uint64_t)__ballot(lane < (uint32_t)kActions && mask[b * kActions + lane] != 0);
    return cand;
}

// gbl_playout_values: flat Monte-Carlo values.  One workgroup of W wavefronts per board (a grid-stride loop over boards).  The
// root position stays in registers (lane c < 27 reads cell c, and three ballots are its planes); the (candidate rank, k) work
// items are dealt round-robin to the 64 W lanes, item i = rank * K + k.  A lane plays its playout in quanta of four plies that
// share one Philox block, and when the playout ends it adds the outcome to the workgroup's LDS counters and starts its next
// item from the root at the next quantum (refill): a wavefront waits for its busiest LANE's sum of playouts, not for the
// longest playout of every round.  The counters go out once per board.  kinv = ceil(2^32 / K): item / K without a divide
// (item < 54 * 4096 = 2^17.8, so the product's error stays below 1 / K).
template <int W>
__global__ __launch_bounds__(64 * W) void k_playout(const int8_t *__restrict__ state, const int8_t *__restrict__ to_move,
                                                    const int8_t *__restrict__ mask, int32_t *__restrict__ wins_out,
                                                    int32_t *__restrict__ losses_out, int32_t *__restrict__ action_out,
                                                    int32_t *__restrict__ plies_out, int64_t n, uint64_t seed, uint64_t env_base,
                                                    uint32_t call, uint32_t K, uint64_t kinv, uint32_t max_plies)
{
    __shared__ uint32_t s_win[kActions], s_loss[kActions], s_plies;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (int64_t b = blockIdx.x; b < n; b += gridDim.x) {
        for (uint32_t j = tid; j < (uint32_t)kActions; j += 64u * W) s_win[j] = s_loss[j] = 0u;
        if (tid == 0) s_plies = 0u;
        const Planes root = board_planes(state, b, lane);
        const int mover = to_move[b] != 0;
        const uint64_t cand = board_candidates(root, mover, mask, b, lane);
        const uint32_t total = (uint32_t)__popcll(cand) * K;
        __syncthreads();  // (counters zeroed)

        uint32_t item = tid, t = 0, plies = 0;
        Planes p = root;
        int side = mover, a = 0;
        uint64_t pid = 0;
        bool fresh = true;
        while (item < total) {
            if (fresh) {  // refill: the next item from the root
                const uint32_t r = (uint32_t)(((uint64_t)item * kinv) >> 32);
                a = (int)kth_bit64(cand, r);
                pid = playout_id(env_base + (uint64_t)b, (uint32_t)a, item - r * K);
                p = root;
                side = mover;
                t = 0;
                fresh = false;
            }
            const Draw4 d = draw_block(seed, pid, playout_ply_index(call, t), kStreamPlayout);  // (t % 4 == 0 here)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!fresh) {
                    const PlayoutEnd e = playout_end(playout_ply(p, side, t, a, d.w[u]), t, mover, max_plies);
                    ++t;
                    if (e.done) {
                        plies += e.plies;
                        if (e.outcome > 0) atomicAdd(&s_win[a], 1u);
                        if (e.outcome < 0) atomicAdd(&s_loss[a], 1u);
                        item += 64u * W;
                        fresh = true;
                    }
                }
            }
        }
        if (plies) atomicAdd(&s_plies, plies);
        __syncthreads();
        if (tid < 64u) {  // wavefront 0: the rows out and the decision (max of the order keys over the wavefront)
            const bool in = lane < (uint32_t)kActions;
            const int w = in ? (int)s_win[lane] : 0, l = in ? (int)s_loss[lane] : 0;
            if (wins_out && in) wins_out[b * kActions + lane] = w;
            if (losses_out && in) losses_out[b * kActions + lane] = l;
            const uint32_t key = wave_max(in && ((cand >> lane) & 1ull) ? playout_key(w, l, (int)lane) : 0u);
            if (lane == 0) {
                if (action_out) action_out[b] = playout_action_of(key);
                if (plies_out) plies_out[b] = (int32_t)s_plies;
            }
        }
        __syncthreads();  // (before the next board zeroes the counters)
    }
}

// Wavefronts per board of k_playout: one where the batch alone fills the chip (16 384 boards are 16 wavefronts per SIMD), more
// for smaller batches -- but never so many that a lane gets fewer than about four playouts of a typical 30-candidate board, or
// the wavefront's time is its unluckiest lane's single long playout.
int playout_waves(int64_t n, int playouts)
{
    int w = 1;
    while (w < 8 && n * (2 * w) <= 16384 && 64 * (2 * w) * 4 <= 30 * playouts) w *= 2;
    return w;
}

// The child list that starts at node `first` (0: empty), walked once by a whole wavefront; the tree is only read.  Lane a keeps the
// child of action a: its index c (0: this lane's action has no child; the root is node 0 and nobody's child), its visits and its wins
// / losses.  A lane without a child holds n = 1, w = l = 0: the selection keys divide by n in every lane before the lanes without a
// child are dropped, so n is never 0; visits() is the count to report.  `first` is wave-uniform and the sibling index goes through
// readfirstlane, so the loop is scalar and the reads broadcast.
struct TreeChild {
    uint32_t c, n, w, l;
    __device__ __forceinline__ bool mine() const { return c != 0u; }
    __device__ __forceinline__ uint32_t visits() const { return c ? n : 0u; }
};

__device__ __forceinline__ TreeChild tree_lane_child(const TreeNode *nodes, uint32_t first, uint32_t lane)
{
    TreeChild r{0u, 1u, 0u, 0u};
    for (uint32_t c = first; c;) {
        const TreeNode k = nodes[c];
        if (lane == tree_action(k)) r = TreeChild{c, k.n, tree_wins(k), tree_losses(k)};
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)k.sibling);
    }
    return r;
}

// The iterations of one board's search, for k_tree and k_collect_search: every thread of the board's W wavefronts calls it.  On entry
// the root node and the sums are zeroed and a barrier has passed; on return the tree is written and a barrier has passed.  count
// (1 on entry) and plies_total (0) count the nodes created and the masked-random plies played.  An iteration:
//   select   every wavefront walks the same path (the tree is only read): the child list of a node once (tree_lane_child), a ballot
//            of the lanes with a child says what is untried, then all lanes compute their key and a butterfly max picks the child;
//            one move_planes per level replays the position;
//   expand   the draw, the move and what it decided, in every lane alike (the node itself is written later, by thread 0);
//   evaluate the P playouts of the leaf dealt to the 64 W lanes, in k_playout's four-ply quanta on one Philox block; wins | losses
//            << 16 and the plies are summed over the wavefront by butterflies and, for W > 1, over the workgroup in LDS counters
//            (two sets, used by alternate iterations, so that zeroing one never races with the adds of the next iteration);
//   back up  thread 0 links the new node and walks to the root, between two barriers.
template <int W>
__device__ __forceinline__ void tree_iterations(TreeNode *const nodes, uint32_t (&s_sum)[2][2], const Planes &root, const int mover,
                                                const uint64_t cand, const uint64_t g, const uint64_t seed, const uint32_t call,
                                                const uint32_t iterations, const uint32_t P, const uint32_t max_plies,
                                                const uint32_t explore, const uint32_t tid, const uint32_t lane, uint32_t &count,
                                                uint32_t &plies_total)
{
    for (uint32_t i = 0; cand && i < iterations; ++i) {
        // 1. select
        uint32_t v = 0, term;
        Planes p = root;
        int side = mover;
        uint64_t cd = cand, untried = 0;
        for (;;) {
            const TreeNode nv = nodes[v];
            term = tree_term(nv);
            if (term) break;
            const TreeChild my = tree_lane_child(nodes, nv.child, lane);
            untried = cd & ~(uint64_t)__ballot(my.mine());
            if (untried) break;
            const uint32_t key = wave_max(my.mine() ? tree_order_key(tree_key(my.w, my.l, my.n, P, nv.n, explore), lane) : 0u);
            const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)(63u - (key & 63u)));
            v = (uint32_t)__builtin_amdgcn_readlane((int)my.c, (int)a);
            move_planes(p, side, a);
            side ^= 1;
            cd = legal54(p, side);
        }
        // 2. expand (the position and what the move decided; the node is linked below)
        const bool grow = term == kTreeOpen;
        uint32_t a_new = 0;
        if (grow) a_new = tree_expand_move(p, side, untried, draw32(seed, tree_pid(g, i, 0), playout_ply_index(call, 0), kStreamTree), term);
        // 3. evaluate
        uint32_t wl = 0, pl = 0;
        if (term == kTreeOpen) {
            uint32_t j = tid, t = 0;
            Planes q = p;
            int s = side;
            uint64_t pid = 0;
            bool fresh = true;
            while (j < P) {
                if (fresh) {
                    pid = tree_pid(g, i, j);
                    q = p;
                    s = side;
                    t = 0;
                    fresh = false;
                }
                const Draw4 d = draw_block(seed, pid, playout_ply_index(call, t), kStreamTree);  // (t % 4 == 0 here)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (!fresh) {
                        const PlayoutEnd e = tree_playout_ply(q, s, side, t, d.w[u], max_plies);
                        ++t;
                        if (e.done) {
                            pl += e.plies;
                            wl += e.outcome > 0 ? 1u : (e.outcome < 0 ? 1u << 16 : 0u);
                            j += 64u * W;
                            fresh = true;
                        }
                    }
                }
            }
            wl = wave_sum(wl);
            pl = wave_sum(pl);
            if (W > 1 && lane == 0) {
                atomicAdd(&s_sum[i & 1u][0], wl);
                atomicAdd(&s_sum[i & 1u][1], pl);
            }
        }
        __syncthreads();  // (every wavefront has read the tree; the sums are complete)
        if (W > 1 && term == kTreeOpen) {
            wl = s_sum[i & 1u][0];
            pl = s_sum[i & 1u][1];
        }
        if (term != kTreeOpen) wl = tree_decided(term, P);
        plies_total += pl;
        // 4. back up
        if (tid == 0) {
            if (W > 1) s_sum[(i & 1u) ^ 1u][0] = s_sum[(i & 1u) ^ 1u][1] = 0u;  // (last read before the previous iteration's second barrier)
            uint32_t leaf = v;
            if (grow) tree_link(nodes, leaf = count, v, a_new, term);
            tree_backup(nodes, leaf, wl & 0xFFFFu, wl >> 16);
        }
        count += grow ? 1u : 0u;
        __syncthreads();  // (the tree is written)
    }
}

// The read-out of a finished search, for k_tree and k_tree_eval (every lane of one wavefront calls it): board b's visits / wins /
// losses rows (each optional) from lanes 0..53, zeros where the root has no child; returns the decision's key in every lane.
__device__ __forceinline__ uint64_t tree_root_out(const TreeNode *nodes, uint32_t lane, int64_t b, int32_t *__restrict__ visits_out,
                                                  int32_t *__restrict__ wins_out, int32_t *__restrict__ losses_out)
{
    const TreeChild c = tree_lane_child(nodes, nodes[0].child, lane);
    if (lane < (uint32_t)kActions) {
        if (visits_out) visits_out[b * kActions + lane] = (int32_t)c.visits();
        if (wins_out) wins_out[b * kActions + lane] = (int32_t)c.w;
        if (losses_out) losses_out[b * kActions + lane] = (int32_t)c.l;
    }
    return wave_max(c.mine() ? tree_final_key(c.n, c.w, c.l, lane) : 0ull);
}

// gbl_tree_search: leaf-parallel UCT.  One workgroup of W wavefronts per board (a grid-stride loop over boards); the tree is an
// array of 16-byte nodes in dynamic LDS, 16 (iterations + 1) bytes, and the root planes stay in registers as in k_playout.  The
// search is tree_iterations; wavefront 0 then writes the root's children out and decides (tree_root_out).
template <int W>
__global__ __launch_bounds__(64 * W) void k_tree(const int8_t *__restrict__ state, const int8_t *__restrict__ to_move,
                                                 const int8_t *__restrict__ mask, int32_t *__restrict__ visits_out,
                                                 int32_t *__restrict__ wins_out, int32_t *__restrict__ losses_out,
                                                 int32_t *__restrict__ action_out, int32_t *__restrict__ nodes_out,
                                                 int32_t *__restrict__ plies_out, int64_t n, uint64_t seed, uint64_t env_base,
                                                 uint32_t call, uint32_t iterations, uint32_t P, uint32_t max_plies, uint32_t explore)
{
    extern __shared__ uint4 s_tree[];
    TreeNode *const nodes = reinterpret_cast<TreeNode *>(s_tree);
    __shared__ uint32_t s_sum[2][2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (int64_t b = blockIdx.x; b < n; b += gridDim.x) {
        if (tid == 0) nodes[0] = TreeNode{};
        if (tid < 4u) (&s_sum[0][0])[tid] = 0u;
        const Planes root = board_planes(state, b, lane);
        const int mover = to_move[b] != 0;
        const uint64_t cand = board_candidates(root, mover, mask, b, lane);
        __syncthreads();  // (root and counters zeroed)
        uint32_t count = 1, plies_total = 0;
        tree_iterations<W>(nodes, s_sum, root, mover, cand, env_base + (uint64_t)b, seed, call, iterations, P, max_plies, explore, tid, lane,
                           count, plies_total);
        if (tid < 64u) {  // wavefront 0: the root's children out, and the decision
            const uint64_t key = tree_root_out(nodes, lane, b, visits_out, wins_out, losses_out);
            if (lane == 0) {
                if (action_out) action_out[b] = tree_action_of(key);
                if (nodes_out) nodes_out[b] = (int32_t)count;
                if (plies_out) plies_out[b] = (int32_t)plies_total;
            }
        }
        __syncthreads();  // (before the next board rewrites the root)
    }
}

// Wavefronts per board of k_tree: a leaf has only `playouts` games to deal, so more than playouts / 64 wavefronts would idle, and
// one is enough once the batch alone gives every SIMD eight wavefronts (8 192 boards).
int tree_waves(int64_t n, int playouts)
{
    int w = 1;
    while (w < 4 && n * (2 * w) <= 8192 && 64 * (2 * w) <= playouts) w *= 2;
    return w;
}

// ---- the integer network (k_evaluate) and the search it guides (k_tree_eval): contract in include/gobblet_hip.h ---------------------
// One evaluation by a whole wavefront; every lane holds the same p / side / cand.
//   layer 1   lane i < H / 4 owns hidden units 4 i .. 4 i + 3: a set observation byte is one coalesced dword per lane of its w1 row
//             (the set bytes come straight from the planes: no observation row is built); the clamped bytes go to s_h, H bytes;
//   layer 2   lane k < 56 owns output k: h as broadcast LDS dwords against its own [j / 4][k] dword of w2, one v_dot4_i32_i8 each;
//   priors    the maximum and the sum over the candidates are wavefront butterflies; the value is lane 54's output.
// Returns lane a's prior byte (0 for a lane outside cand), its output (0 for lanes >= 56) and q in every lane.
struct WaveEval {
    uint32_t pi;
    int32_t o, q;
};

__device__ __forceinline__ WaveEval wave_evaluate(const EvalNet &net, const Planes &p, int side, uint64_t cand, uint32_t *s_h, uint32_t lane)
{
    if (4u * lane < (uint32_t)net.hidden) s_h[lane] = eval_hidden4(net, p, side, 4u * lane);
    wave_lds_fence();
    const int32_t o = lane < (uint32_t)kEvalOutputs ? eval_output(net, s_h, lane) : 0;
    wave_lds_fence();  // (h is read before the next evaluation overwrites it)
    const bool in = (cand >> lane) & 1ull;
    const int32_t l = o >> net.shift_p;
    const int32_t lmax = wave_max<int32_t>(in ? l : INT32_MIN);
    const uint32_t e = in ? eval_exp2(lmax, l) : 0u;
    const uint32_t sum = wave_sum(e);
    return WaveEval{in ? eval_prior(e, sum) : 0u, o, eval_value(net, __builtin_amdgcn_readlane(o, kEvalValue))};
}

// gbl_evaluate: the network alone.  One wavefront per board (a grid-stride loop over boards).
__global__ __launch_bounds__(64) void k_evaluate(const int8_t *__restrict__ state, const int8_t *__restrict__ to_move,
                                                 const int8_t *__restrict__ mask, const EvalNet net, uint8_t *__restrict__ priors_out,
                                                 int32_t *__restrict__ value_out, int32_t *__restrict__ logits_out, int64_t n)
{
    __shared__ uint32_t s_h[kEvalMaxHidden / 4];
    const uint32_t lane = threadIdx.x;
    for (int64_t b = blockIdx.x; b < n; b += gridDim.x) {
        const Planes p = board_planes(state, b, lane);
        const int mover = to_move[b] != 0;
        const WaveEval r = wave_evaluate(net, p, mover, board_candidates(p, mover, mask, b, lane), s_h, lane);
        if (lane < (uint32_t)kActions) priors_out[b * kActions + lane] = (uint8_t)r.pi;
        if (logits_out && lane < (uint32_t)kEvalOutputs) logits_out[b * kEvalOutputs + lane] = r.o;
        if (lane == 0) value_out[b] = r.q;
    }
}

// The evaluator-guided search of one board, for k_tree_eval and k_collect_eval: every lane of the board's one wavefront calls it,
// with the same root / mover / cand.  LDS traffic of one wavefront lands in order, so the tree needs no workgroup barrier, only
// wave_lds_fence.  nodes: iterations + 1 nodes at least; pri: a 56-byte prior row per node.  On return the tree is written and
// fenced, count is the nodes created (the root included), and the root's evaluation comes back: lane a's prior byte and q.  The
// root is created before iteration 0; an iteration:
//   select   k_tree's walk -- the child list of a node once, tree_lane_child -- plus one byte of the node's prior
//            row per lane; every lane computes its action's key, a butterfly max picks, one move_planes per level replays the position;
//   expand   the move and what it decided in every lane alike; lane 0 links the node;
//   evaluate wave_evaluate on the new child's position, its prior row stored beside the node;
//   back up  lane 0 walks to the root.
// noise: the root noise of this search (w == 0: none, nothing is drawn); NOISE = false compiles it out, so that the kernels without
// it are the code they were.  mixed: lane a's byte of the row the root keeps -- pi' where there is noise, the network's byte
// otherwise; the returned pi is the network's either way.
struct RootNoise {
    uint32_t w;
    uint64_t seed, g;
    uint32_t q;
};

// The Gumbel root rule of one search (include/gobblet_hip.h, "Gumbel root search"; GUMBEL = false compiles it out, and G.considered == 0
// is a side that searches by the keys).  The wavefront's whole state: lane a keeps g_a and g_a + l_a, the considered set A is a ballot
// mask, and the schedule's phase count and target are wave-uniform locals of tree_eval_iterations -- no LDS.
struct WaveGumbel {
    GumbelArgs G;
    uint64_t seed, g;
    uint32_t q;
    int32_t gum, gl;  // (out) this lane's g_a and g_a + l_a; 0 outside the candidates
    uint64_t A;       // (out) the considered set after the last halving; 0 where the rule did not run
};

// the k lanes of A with the largest keys, as a mask (the keys differ; key == 0 outside A): a lane counts the keys above its own
__device__ __forceinline__ uint64_t wave_gumbel_keep(uint32_t key, uint64_t A, uint32_t k)
{
    uint32_t above = 0;
    for (uint64_t i = A; i; i &= i - 1) {
        const int j = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(i));
        above += (uint32_t)__builtin_amdgcn_readlane((int)key, j) > key ? 1u : 0u;
    }
    return (uint64_t)__ballot(key != 0u && above < k);
}

// after the last iteration (the rule ran: gb.A != 0): the decision in every lane, and lane a's byte of the target row.  c: the lane's
// root child, as tree_lane_child gives it.
struct GumbelOut {
    int action;
    uint32_t target;
};

__device__ __forceinline__ GumbelOut wave_gumbel_finish(const WaveGumbel &gb, const TreeChild &c, uint64_t cand, int32_t q_root, uint32_t lane)
{
    const bool in = (cand >> lane) & 1ull, in_a = (gb.A >> lane) & 1ull;
    const uint32_t max_n = wave_max(c.visits());
    const int32_t sigma = gumbel_sigma(gb.G, max_n, gumbel_mean(c.mine(), c.w, c.l, c.n, q_root));
    const int32_t t = gb.gl - gb.gum + sigma;
    const int32_t tmax = wave_max<int32_t>(in ? t : INT32_MIN);
    const uint32_t e = in ? eval_exp2(tmax, t) : 0u;
    const uint32_t sum = wave_sum(e);
    const uint32_t key = wave_max(in_a ? gumbel_final_key(c.visits(), gb.gl + sigma, lane) : 0u);
    return GumbelOut{gumbel_action_of(key), in ? eval_prior(e, sum) : 0u};
}

// ... and the read-out of a finished search: action -1 and a zero row where the rule did not run (gb.A == 0: a root without candidates)
__device__ __forceinline__ GumbelOut wave_gumbel_out(const WaveGumbel &gb, const TreeNode *nodes, uint64_t cand, int32_t q_root, uint32_t lane)
{
    GumbelOut out{-1, 0u};
    if (gb.A) out = wave_gumbel_finish(gb, tree_lane_child(nodes, nodes[0].child, lane), cand, q_root, lane);
    return out;
}

template <bool NOISE, bool GUMBEL = false>
__device__ __forceinline__ WaveEval tree_eval_iterations(TreeNode *const nodes, uint8_t *const pri, uint32_t *const s_h, const EvalNet &net,
                                                         const Planes &root, const int mover, const uint64_t cand, const uint32_t iterations,
                                                         const uint32_t explore, const uint32_t lane, uint32_t &count, const RootNoise &noise,
                                                         uint32_t &mixed, WaveGumbel *const gb = nullptr)
{
    if (lane == 0) nodes[0] = TreeNode{};
    const WaveEval at_root = wave_evaluate(net, root, mover, cand, s_h, lane);
    mixed = at_root.pi;
    if (NOISE && noise.w && cand) {  // (wave-uniform) the root's row alone: lane a draws its word, the noise row is the prior rule over the words
        const bool in = (cand >> lane) & 1ull;
        const int32_t l = noise_logit(noise.seed, noise.g, noise.q, lane);
        const int32_t lmax = wave_max<int32_t>(in ? l : INT32_MIN);
        const uint32_t e = in ? eval_exp2(lmax, l) : 0u;
        const uint32_t sum = wave_sum(e);
        mixed = in ? noise_mix(at_root.pi, eval_prior(e, sum), noise.w) : 0u;
    }
    if (lane < (uint32_t)kEvalOutputs) pri[lane] = (uint8_t)mixed;
    wave_lds_fence();  // (the root is written)
    count = 1;
    bool rule = false;          // (wave-uniform) the root follows the Gumbel rule
    uint32_t phases = 1, T = 0;  // the schedule: P and the visit target of the next halving
    if constexpr (GUMBEL) {
        rule = gb->G.considered != 0u && cand != 0ull;
        gb->gum = gb->gl = 0;
        gb->A = 0ull;
        if (rule) {
            const bool in = (cand >> lane) & 1ull;
            const int32_t l = at_root.o >> net.shift_p;
            const int32_t lmax = wave_max<int32_t>(in ? l : INT32_MIN);
            if (gb->G.noise) gb->gum = in ? gumbel_draw(gb->seed, gb->g, gb->q, lane) : 0;
            gb->gl = in ? gb->gum + gumbel_logit(lmax, l) : 0;
            const uint32_t c = (uint32_t)__popcll(cand), m = gb->G.considered < c ? gb->G.considered : c;
            gb->A = wave_gumbel_keep(in ? gumbel_rank_key(gb->gl, lane) : 0u, cand, m);
            phases = gumbel_phases(m);
            T = gumbel_step(iterations, phases, m);
        }
    }
    for (uint32_t i = 0; cand && i < iterations; ++i) {
        // 1. select
        uint32_t v = 0, term, a_new = 0;
        Planes p = root;
        int side = mover;
        uint64_t cd = cand;
        bool grow = false;
        for (;;) {
            const TreeNode nv = nodes[v];
            term = tree_term(nv);
            if (term) break;
            const TreeChild my = tree_lane_child(nodes, nv.child, lane);
            const uint32_t pi = lane < (uint32_t)kEvalOutputs ? pri[v * kEvalOutputs + lane] : 0u;
            uint32_t key;
            if (GUMBEL && rule && v == 0u) {  // the root: halve where the schedule says so, then the least visited action of A
                uint64_t A = gb->A;
                const bool in_a = (A >> lane) & 1ull;
                const uint32_t size = (uint32_t)__popcll(A);
                if (size > 2u && !__ballot(in_a && my.visits() < T)) {
                    const int32_t sigma = gumbel_sigma(gb->G, wave_max(my.visits()), gumbel_mean(my.mine(), my.w, my.l, my.n, at_root.q));
                    A = wave_gumbel_keep(in_a ? gumbel_rank_key(gb->gl + sigma, lane) : 0u, A, gumbel_kept(size));
                    gb->A = A;
                    T += gumbel_step(iterations, phases, (uint32_t)__popcll(A));
                }
                key = wave_max(((A >> lane) & 1ull) ? gumbel_pick_key(my.visits(), gb->gl, lane) : 0u);
            } else {
                key = wave_max(((cd >> lane) & 1ull) ? tree_order_key(tree_eval_key(my.mine(), my.w, my.l, my.n, nv.n, pi, explore), lane) : 0u);
            }
            a_new = (uint32_t)__builtin_amdgcn_readfirstlane((int)(63u - (key & 63u)));
            const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)my.c, (int)a_new);
            if (!c) {
                grow = true;
                break;
            }
            move_planes(p, side, a_new);
            side ^= 1;
            v = c;
            cd = legal54(p, side);
        }
        // 2. expand and evaluate
        uint32_t leaf = v;
        if (grow) {
            term = tree_move_into(p, side, a_new);
            leaf = count++;
            if (lane == 0) tree_link(nodes, leaf, v, a_new, term);
        }
        uint32_t wl = tree_decided(term, kTreeEvalP);
        if (grow && term == kTreeOpen) {
            const WaveEval r = wave_evaluate(net, p, side, legal54(p, side), s_h, lane);
            if (lane < (uint32_t)kEvalOutputs) pri[leaf * kEvalOutputs + lane] = (uint8_t)r.pi;
            wl = tree_eval_outcome(r.q);
        }
        // 3. back up
        if (lane == 0) tree_backup(nodes, leaf, wl & 0xFFFFu, wl >> 16);
        wave_lds_fence();  // (the tree is written)
    }
    return at_root;
}

// gbl_tree_search_eval: k_tree's tree with a network leaf.  One wavefront per board (a grid-stride loop over boards).  The tree is
// (iterations + 1) 16-byte nodes followed by (iterations + 1) 56-byte prior rows in dynamic LDS; the root planes stay in registers.
// The search is tree_eval_iterations; the wavefront then writes the root's children out and decides (tree_root_out).
// GUMBEL: gbl_tree_search_gumbel -- the root follows the Gumbel rule (tree_eval_iterations<.., true>), the decision and the target row
// come from wave_gumbel_finish on the root's children that tree_root_out has just read out.
struct GumbelOutputs {  // (empty in the instantiations without the rule)
    uint8_t *target;
    int16_t *gumbel;
    GumbelArgs G;
};

template <bool NOISE, bool GUMBEL = false>
__global__ __launch_bounds__(64) void k_tree_eval(const int8_t *__restrict__ state, const int8_t *__restrict__ to_move,
                                                  const int8_t *__restrict__ mask, const EvalNet net, int32_t *__restrict__ visits_out,
                                                  int32_t *__restrict__ wins_out, int32_t *__restrict__ losses_out,
                                                  int32_t *__restrict__ action_out, int32_t *__restrict__ nodes_out,
                                                  int32_t *__restrict__ root_value_out, uint8_t *__restrict__ root_priors_out, int64_t n,
                                                  uint32_t iterations, uint32_t explore, uint8_t *__restrict__ root_mixed_out, uint32_t noise,
                                                  uint64_t seed, uint64_t env_base, uint32_t call, const GumbelOutputs gum)
{
    extern __shared__ uint4 s_tree[];
    TreeNode *const nodes = reinterpret_cast<TreeNode *>(s_tree);
    uint8_t *const pri = reinterpret_cast<uint8_t *>(nodes + iterations + 1);
    __shared__ uint32_t s_h[kEvalMaxHidden / 4];
    const uint32_t lane = threadIdx.x;
    for (int64_t b = blockIdx.x; b < n; b += gridDim.x) {
        const Planes root = board_planes(state, b, lane);
        const int mover = to_move[b] != 0;
        const uint64_t cand = board_candidates(root, mover, mask, b, lane);
        uint32_t count, mixed;
        WaveGumbel gb{gum.G, seed, env_base + (uint64_t)b, call, 0, 0, 0ull};
        const WaveEval at_root = tree_eval_iterations<NOISE, GUMBEL>(nodes, pri, s_h, net, root, mover, cand, iterations, explore, lane, count,
                                                                     RootNoise{noise, seed, env_base + (uint64_t)b, call}, mixed, &gb);
        const uint64_t key = tree_root_out(nodes, lane, b, visits_out, wins_out, losses_out);
        int action = GUMBEL ? -1 : tree_action_of(key);
        if constexpr (GUMBEL) {
            const GumbelOut out = wave_gumbel_out(gb, nodes, cand, at_root.q, lane);
            action = out.action;
            if (lane < (uint32_t)kActions) {
                if (gum.target) gum.target[b * kActions + lane] = (uint8_t)out.target;
                if (gum.gumbel) gum.gumbel[b * kActions + lane] = (int16_t)gb.gum;
            }
        }
        if (root_priors_out && lane < (uint32_t)kActions) root_priors_out[b * kActions + lane] = (uint8_t)at_root.pi;
        if (NOISE && root_mixed_out && lane < (uint32_t)kActions) root_mixed_out[b * kActions + lane] = (uint8_t)mixed;
        if (lane == 0) {
            if (action_out) action_out[b] = action;
            if (nodes_out) nodes_out[b] = (int32_t)count;
            if (root_value_out) root_value_out[b] = at_root.q;
        }
        wave_lds_fence();  // (before the next board rewrites the root)
    }
}

// gbl_collect_search: whole games with the tree search on either or both sides, every ply materialised.  One workgroup of W
// wavefronts per board (a grid-stride loop over boards) with the ply loop INSIDE: a board whose search walks into decided nodes
// and plays nothing goes on to its next ply while its neighbours still play iterations x playouts games -- no ply of any board
// waits for the slowest board's search, and neither a second launch nor the action's round trip through HBM lies between a
// search and its step.  Between two searches only the planes, the mover, the turn and the done flag are live, all wave-uniform
// (every wavefront replays the same ply; wavefront 0 stores).  A tree side's ply:
//   search   the root node is zeroed, then tree_iterations -- the tree in 16 (iterations + 1) bytes of dynamic LDS, rebuilt from
//            an empty root on every ply (call q's search IS gbl_tree_search(call = q));
//   decide   lane a reads the root's child of action a; butterflies give the decision's key and the value sum, a prefix sum over
//            the lanes the visit-proportional draw of a game's first plies (stream kStreamVisit);
//   step     play_ply / next_turn / next_mask on the planes; the state row is rebuilt from them once, after the last ply;
//   store    the scalars from lane 0, the visits row from lanes 0..53, and the mask and observation rows built in LDS by
//            mask_row_part<4> / obs_scatter_part<4> on lanes 0..3 and stored a byte per lane, all non-temporally.
struct SearchTraj {
    int32_t *actions;
    int8_t *winner, *reward, *done, *to_move, *mask, *obs;
    int16_t *visits;
    int32_t *value, *nodes;
    int8_t *how, *mover;
};

// What the self-play kernels (k_collect_search and the evaluator family of five) do between a search and the next one; wavefront 0's lanes call
// search_decide and store_search_ply, every thread of the board's workgroup the other two.
//
// decide: lane a reads the root's child of action a; butterflies give the decision's key and the value sum; `sampled` (a game's
// first plies): the visit-proportional draw on stream kStreamVisit, by a prefix sum of the visits over the lanes.
struct SearchDecision {
    int action, how, value;
    uint32_t my_n;  // (the visits of this lane's action)
};

__device__ __forceinline__ SearchDecision search_decide(const TreeNode *nodes, uint32_t lane, bool sampled, uint64_t seed, uint64_t g, uint32_t q)
{
    const TreeChild c = tree_lane_child(nodes, nodes[0].child, lane);
    SearchDecision d{0, kHowSearch, (int)wave_sum(c.w - c.l), c.visits()};
    d.action = tree_action_of(wave_max(c.mine() ? tree_final_key(c.n, c.w, c.l, lane) : 0ull));
    if (sampled) {
        uint32_t run = c.visits();  // (the running sum of the visits through this lane's action)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t below = (uint32_t)__shfl_up((int)run, o);
            run += lane >= (uint32_t)o ? below : 0u;
        }
        const uint32_t S = (uint32_t)__builtin_amdgcn_readlane((int)run, 63);
        const uint32_t k = __umulhi(draw32(seed, g, q, kStreamVisit), S);
        const uint64_t over = (uint64_t)__ballot(run > k);
        d.action = over ? (int)__builtin_ctzll(over) : -1;
        d.how = kHowSearchSampled;
    }
    return d;
}

// step: play_ply / next_turn on the planes with auto-reset, everything left wave-uniform; the tallies of the board's games
struct SearchBoard {
    Planes p;
    int mover, tabs, dn;
    uint32_t games, w1, w2;
};

__device__ __forceinline__ Ply search_step(SearchBoard &B, uint64_t legal, int action, int illegal_mode, int &winner)
{
    const Ply y = play_ply(B.p, NoRow{}, B.mover, legal, action, illegal_mode);
    B.dn = uniform(y.terminal ? 1 : 0);
    if (B.dn) {  // raw_env.reset, gobblet.py:275-290
        B.p = Planes{0u, 0u, 0u};
        B.mover = 0;
    }
    B.p = Planes{(uint32_t)uniform((int)B.p.nz), (uint32_t)uniform((int)B.p.neg), (uint32_t)uniform((int)B.p.odd)};
    B.mover = uniform(B.mover);
    B.tabs = uniform(next_turn(B.tabs, y, 1));
    winner = uniform(y.winner);
    B.games += (uint32_t)B.dn;
    B.w1 += winner == 1;
    B.w2 += winner == -1;
    return y;
}

// store: the scalars from lane 0, the visits row from lanes 0..53, and the mask and observation rows built in LDS by
// mask_row_part<4> / obs_scatter_part<4> on lanes 0..3 and stored a byte per lane, all non-temporally.  B: the board AFTER the ply.
__device__ __forceinline__ void store_search_ply(const SearchTraj &T, int64_t at, uint32_t lane, uint32_t *s_mask, uint32_t *s_obs,
                                                 const SearchBoard &B, const Ply &y, int winner, int action, int value, uint32_t count,
                                                 int how, int who, uint32_t my_n)
{
    if (lane == 0) {
        if (T.actions) T.actions[at] = action;
        if (T.winner) T.winner[at] = (int8_t)winner;
        if (T.reward) reinterpret_cast<uint16_t *>(T.reward)[at] = (uint16_t)((y.r0 & 0xFF) | ((y.r1 & 0xFF) << 8));
        if (T.done) T.done[at] = (int8_t)B.dn;
        if (T.to_move) T.to_move[at] = (int8_t)B.mover;
        if (T.value) T.value[at] = value;
        if (T.nodes) T.nodes[at] = (int32_t)count;
        if (T.how) T.how[at] = (int8_t)how;
        if (T.mover) T.mover[at] = (int8_t)who;
    }
    if (T.visits && lane < (uint32_t)kActions) __builtin_nontemporal_store((int16_t)my_n, T.visits + at * kActions + lane);
    if (T.mask) {
        if (lane < 4u) mask_row_part<4>(reinterpret_cast<uint8_t *>(s_mask), next_mask(B.p, B.mover, B.dn, 1), (int)lane);
        wave_lds_fence();
        if (lane < (uint32_t)kActions)
            __builtin_nontemporal_store(reinterpret_cast<const int8_t *>(s_mask)[lane], T.mask + at * kActions + lane);
        wave_lds_fence();
    }
    if (T.obs) {
        if (lane < 32u) s_obs[lane] = 0u;
        wave_lds_fence();
        if (lane < 4u) obs_scatter_part<4>(reinterpret_cast<uint8_t *>(s_obs), B.p, B.mover, (int)lane);
        wave_lds_fence();
        const int8_t *row = reinterpret_cast<const int8_t *>(s_obs);
        __builtin_nontemporal_store(row[lane], T.obs + at * kObs + lane);
        if (lane + 64u < (uint32_t)kObs) __builtin_nontemporal_store(row[lane + 64u], T.obs + at * kObs + lane + 64u);
        wave_lds_fence();
    }
}

// ... and after the last ply: the state row from the planes (planes_to_row, a cell per lane), the board's scalars and its tallies
__device__ __forceinline__ void store_search_board(int8_t *__restrict__ state, int8_t *__restrict__ to_move, int8_t *__restrict__ done,
                                                   int32_t *__restrict__ turn, int64_t *__restrict__ counters, int64_t b, uint32_t tid,
                                                   const SearchBoard &B, uint32_t plies)
{
    if (tid < (uint32_t)kCells) {
        const uint32_t nz = (B.p.nz >> tid) & 1u, ng = (B.p.neg >> tid) & nz, od = (B.p.odd >> tid) & nz;
        const uint32_t v = nz * (tid >= 18u ? 6u : (tid >= 9u ? 4u : 2u)) - od;
        state[b * kCells + tid] = (int8_t)(ng ? 0u - v : v);
    }
    if (tid == 0) {
        to_move[b] = (int8_t)B.mover;
        done[b] = (int8_t)B.dn;
        if (turn) turn[b] = B.tabs;
        if (counters) tally_flush(counters, b, 1, plies, B.games, B.w1, B.w2);
    }
}

// What a ply's search leaves for the stores (all zero on a masked-random ply): the decision, the nodes created and, from the
// evaluator-guided search alone, the root's q and this lane's byte of the root's prior row.
struct SearchPly {
    SearchDecision d;
    uint32_t count, pi;
    int root_q;
};

// The boards and plies of a self-play launch, for k_collect_search and the evaluator family (every thread of the workgroup calls it; the
// host flavour's selfplay_boards is the same loop).  search(B, who, legal, g, q, S): the mover's search of call q on board B -- false
// where the masked-random sampler moves, else it fills S (the decision by search_decide) and returns after whatever keeps the next
// search's writes to the tree behind this one's reads.  stored(at, S): wavefront 0, after the ply's cell `at` is written -- a
// kernel's own extra trajectory arrays.  Both are lambdas of the calling kernel and are inlined here.
template <typename Search, typename Stored>
__device__ __forceinline__ void search_plies(int8_t *__restrict__ state, int8_t *__restrict__ to_move, int8_t *__restrict__ done,
                                             int32_t *__restrict__ turn, int64_t *__restrict__ counters, int64_t n, uint64_t seed,
                                             uint64_t env_base, const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies,
                                             int64_t ply_stride, int64_t tile_stride, const SearchTraj &T, int illegal_mode, uint32_t *s_mask,
                                             uint32_t *s_obs, Search &&search, Stored &&stored)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (ply_dev) ply0 += *ply_dev;
    for (int64_t b = blockIdx.x; b < n; b += gridDim.x) {
        SearchBoard B{board_planes(state, b, lane), to_move[b] != 0, turn ? turn[b] : 0, 0, 0u, 0u, 0u};
        const uint64_t g = env_base + (uint64_t)b;
        const int64_t cell0 = (b >> 6) * tile_stride + (b & 63);
        for (uint32_t t = 0; t < plies; ++t) {
            const uint32_t q = ply0 + t;
            const int who = B.mover;
            const uint64_t legal = legal54(B.p, who);
            SearchPly S{};
            if (!search(B, who, legal, g, q, S)) S.d.action = pick54(legal, draw32(seed, g, q));
            const int action = uniform(S.d.action);
            int winner;
            const Ply y = search_step(B, legal, action, illegal_mode, winner);
            if (tid < 64u) {  // wavefront 0: the ply's outputs
                const int64_t at = (int64_t)t * ply_stride + cell0;
                store_search_ply(T, at, lane, s_mask, s_obs, B, y, winner, action, S.d.value, S.count, S.d.how, who, S.d.my_n);
                stored(at, S);
            }
        }
        store_search_board(state, to_move, done, turn, counters, b, tid, B, plies);
    }
}

template <int W>
__global__ __launch_bounds__(64 * W) void k_collect_search(int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n, uint64_t seed,
                                                           uint64_t env_base, const uint32_t *__restrict__ ply_dev, uint32_t ply0,
                                                           uint32_t plies, int8_t *__restrict__ done, int64_t ply_stride, int64_t tile_stride,
                                                           SearchTraj T, int policy0, int policy1, uint32_t iterations0, uint32_t iterations1,
                                                           uint32_t playouts0, uint32_t playouts1, uint32_t max_plies, uint32_t explore,
                                                           int sample_plies, int illegal_mode, int64_t *__restrict__ counters,
                                                           int32_t *__restrict__ turn)
{
    extern __shared__ uint4 s_tree[];
    TreeNode *const nodes = reinterpret_cast<TreeNode *>(s_tree);
    __shared__ uint32_t s_sum[2][2];
    __shared__ uint32_t s_obs[32], s_mask[16];  // the ply's observation row (117 bytes) and mask row (54)
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    search_plies(
        state, to_move, done, turn, counters, n, seed, env_base, ply_dev, ply0, plies, ply_stride, tile_stride, T, illegal_mode, s_mask, s_obs,
        [&](const SearchBoard &B, int who, uint64_t legal, uint64_t g, uint32_t q, SearchPly &S) {
            if ((who ? policy1 : policy0) != kPolicyTree) return false;
            if (tid == 0) nodes[0] = TreeNode{};
            if (tid < 4u) (&s_sum[0][0])[tid] = 0u;
            __syncthreads();  // (root and counters zeroed)
            uint32_t plies_total = 0;
            S.count = 1;
            tree_iterations<W>(nodes, s_sum, B.p, who, legal, g, seed, q, who ? iterations1 : iterations0, who ? playouts1 : playouts0,
                               max_plies, explore, tid, lane, S.count, plies_total);
            S.d = search_decide(nodes, lane, B.tabs < sample_plies, seed, g, q);
            __syncthreads();  // (every wavefront has read the root's children before the next search rewrites the tree)
            return true;
        },
        [](int64_t, const SearchPly &) {});
}

// the mover's network, picked wave-uniformly field by field: the two structs stay in SGPRs
__device__ __forceinline__ EvalNet eval_net_pick(const EvalNet &a, const EvalNet &b, int second)
{
    return EvalNet{second ? b.w1 : a.w1, second ? b.b1 : a.b1, second ? b.w2 : a.w2, second ? b.b2 : a.b2, second ? b.hidden : a.hidden,
                   second ? b.shift1 : a.shift1, second ? b.shift_p : a.shift_p, second ? b.shift_v : a.shift_v};
}

// gbl_outcome_targets: one reverse pass over the plies per board, a lane per board and a wavefront per tile of 64 boards -- in both
// layouts the 64 lanes of a ply read and write consecutive elements.  A ply's loads do not depend on the pass's state (the reward
// is read whether or not the game ended there), so the unrolled loop keeps several plies' loads in flight: 4 bytes in and up to 3
// out per cell, memory-bound.
__global__ __launch_bounds__(64) void k_outcome_targets(const int8_t *__restrict__ done_t, const int8_t *__restrict__ reward_t,
                                                        const int8_t *__restrict__ mover_t, int8_t *__restrict__ z_t,
                                                        int16_t *__restrict__ left_t, int64_t n, int64_t ntiles, int64_t ply_stride,
                                                        int64_t tile_stride, uint32_t plies)
{
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tile * kTile + (int64_t)threadIdx.x >= n) continue;
        const int64_t cell0 = tile * tile_stride + threadIdx.x;
        uint32_t rw = 0;  // the two rewards of the nearest game end at or after t
        int left = -1;    // ... and how many plies ahead it lies
#pragma unroll 4
        for (uint32_t t = plies; t-- > 0;) {
            const int64_t at = (int64_t)t * ply_stride + cell0;
            const int d = done_t[at], m = mover_t[at];
            const uint32_t r = reinterpret_cast<const uint16_t *>(reward_t)[at];
            left = d ? 0 : (left >= 0 ? left + 1 : left);
            rw = d ? r : rw;
            z_t[at] = (int8_t)(left < 0 ? kZOpen : (int)(int8_t)(m ? rw >> 8 : rw & 0xFFu));
            if (left_t) left_t[at] = (int16_t)left;
        }
    }
}

// gbl_symmetry_apply: a tile of 64 boards per wavefront, one row type after the other over the LDS-image path -- the tile's rows in
// as 16-byte vectors, lane l permutes ITS row from the one image into the other (constant indices: the rule's divisions fold away,
// what is left per byte is a nibble of sigma^-1 and an LDS byte each way), the tile out as 16-byte vectors.
struct SymRows {
    const int8_t *state_in, *obs_in, *mask_in;
    const int16_t *visits_in;
    const uint8_t *priors_in;
    const int32_t *actions_in;
    int8_t *state_out, *obs_out, *mask_out;
    int16_t *visits_out;
    uint8_t *priors_out;
    int32_t *actions_out;
};

// one row type of the tile: `row(in, out)` moves the lane's ROWB bytes
template <int ROWB, typename Row>
__device__ __forceinline__ void sym_tile(const void *in, void *out, uint32_t *s_in, uint32_t *s_out, const Lane &L, Row row)
{
    tile_in<ROWB>(static_cast<const int8_t *>(in) + L.tile * (kTile * ROWB), s_in, L.lane, L.rows);
    wave_lds_fence();
    row(reinterpret_cast<const int8_t *>(s_in) + L.lane * ROWB, reinterpret_cast<int8_t *>(s_out) + L.lane * ROWB);
    wave_lds_fence();
    tile_out<ROWB, kStoreStream>(static_cast<int8_t *>(out) + L.tile * (kTile * ROWB), s_out, L.lane, L.rows);
    wave_lds_fence();  // (the images are reused by the next row type)
}

__global__ __launch_bounds__(64) void k_symmetry_apply(const int16_t *__restrict__ sym, int sym_all, const int8_t *__restrict__ agent,
                                                       SymRows R, int64_t n, int64_t ntiles)
{
    __shared__ uint32_t s_in[image_words<kObs>()];
    __shared__ uint32_t s_out[image_words<kObs>()];
    Lane L;
    if (!lane_setup(L, n, ntiles)) return;
    // (lanes past the end of a ragged last tile permute whatever the image holds with the identity: nothing of theirs is stored)
    const Sym S = sym_of((uint32_t)(sym ? (L.valid ? (int)sym[L.b] : 0) : sym_all) & 511u);
    const uint32_t m = agent && L.valid ? agent[L.b] != 0 : 0u;
    if (R.state_in) sym_tile<kCells>(R.state_in, R.state_out, s_in, s_out, L, [&](const int8_t *i, int8_t *o) { sym_state_row(i, o, S); });
    if (R.obs_in) sym_tile<kObs>(R.obs_in, R.obs_out, s_in, s_out, L, [&](const int8_t *i, int8_t *o) { sym_obs_row(i, o, S, m); });
    if (R.mask_in) sym_tile<kActions>(R.mask_in, R.mask_out, s_in, s_out, L, [&](const int8_t *i, int8_t *o) { sym_action_row(i, o, S, m); });
    if (R.priors_in) sym_tile<kActions>(R.priors_in, R.priors_out, s_in, s_out, L, [&](const int8_t *i, int8_t *o) { sym_action_row(i, o, S, m); });
    if (R.visits_in)
        sym_tile<2 * kActions>(R.visits_in, R.visits_out, s_in, s_out, L, [&](const int8_t *i, int8_t *o) {
            sym_action_row(reinterpret_cast<const int16_t *>(i), reinterpret_cast<int16_t *>(o), S, m);
        });
    if (R.actions_in && L.valid) R.actions_out[L.b] = sym_action_any(S, m, R.actions_in[L.b]);
}

// gbl_training_batch: 64 samples per wavefront.
//   1. Lane l draws sample l: up to 16 attempts of one generator block, two byte loads and the 27 dwords of the visits row each
//      (the loop ends when every lane has its cell), then writes the sample's scalars and leaves its source cells, sigma^-1 and
//      swap bits in LDS.
//   2. Row type after row type, the 64 output rows are gathered into ONE LDS image, permuted on the way in: the wavefront walks
//      the samples, lane k fetching the source element of output element k (and k + 64 of an observation row) of sample r -- k is the
//      lane's own, so its cell and channel are computed once, and per sample what is left is a nibble of sigma^-1 and a swap bit.
//      A row's 117 / 54 / 108 source bytes lie in one or two 128-byte lines; four samples' loads are in flight at a time.
//   3. The image -- a contiguous tile of the output -- leaves as whole 16-byte vectors (tile_out, ragged last tile as elsewhere).
struct BatchArgs {
    const int8_t *obs, *mask;
    const int16_t *visits;
    const int8_t *z, *done, *mover;
    int8_t *obs_out, *mask_out;
    int16_t *visits_out;
    int8_t *z_out;
    int32_t *index_out;
    int16_t *sym_out;
    int64_t n, ply_stride, tile_stride, batch, ntiles;
    uint64_t seed, sample_base;
    uint32_t plies, call, sym_mask;
};

// rows `ROWS` of element type T and E elements: element k of sample r from src[cell_r * PITCH + from(r, k)], zeros for a failed sample
// (PITCH: the source's row pitch in elements -- E in a trajectory array, a whole line in the replay ring)
template <typename T, int E, int PITCH, typename From>
__device__ __forceinline__ void batch_gather(const T *__restrict__ src, T *img, const int64_t *s_cell, int rows, uint32_t k, From from)
{
    if (k >= (uint32_t)E) return;
#pragma unroll 4
    for (int r = 0; r < rows; ++r) {
        const int64_t c = s_cell[r];
        const T v = src[(c >= 0 ? c : 0) * PITCH + from(r, k)];  // (a failed sample reads cell 0 and drops it: no branch around the load)
        img[r * E + (int)k] = c >= 0 ? v : (T)0;
    }
}

// Phases 2 and 3 of a batch kernel (k_training_batch, k_replay_batch): the 64 output rows of each type gathered into the one LDS image
// under the samples' symmetries (s_inv, s_sw = swap bits | mover << 6) and stored as a tile.  s_prev / s_at: the source rows of the
// observation and the mask / of the visits (-1: a failed sample); the pitches are the sources' row pitches in elements.
template <int OBS_PITCH, int MASK_PITCH, int VISITS_PITCH>
__device__ __forceinline__ void batch_rows(const int8_t *__restrict__ obs, const int8_t *__restrict__ mask, const int16_t *__restrict__ visits,
                                           int8_t *obs_out, int8_t *mask_out, int16_t *visits_out, uint32_t *s_img, const int64_t *s_at,
                                           const int64_t *s_prev, const uint64_t *s_inv, const uint32_t *s_sw, const Lane &L)
{
    const uint32_t k = (uint32_t)L.lane;
    const auto sym_r = [&](int r) { return Sym{0ull, s_inv[r], s_sw[r] & 63u}; };
    if (obs_out) {
        int8_t *img = reinterpret_cast<int8_t *>(s_img);
        const auto from = [&](int r, uint32_t e) { return sym_obs_src(sym_r(r), s_sw[r] >> 6, e); };
        batch_gather<int8_t, kObs, OBS_PITCH>(obs, img, s_prev, L.rows, k, from);
        batch_gather<int8_t, kObs, OBS_PITCH>(obs, img, s_prev, L.rows, k + 64u, from);
        wave_lds_fence();
        tile_out<kObs, kStoreStream>(obs_out + L.tile * (kTile * kObs), s_img, L.lane, L.rows);
        wave_lds_fence();
    }
    const auto from = [&](int r, uint32_t e) { return sym_action_src(sym_r(r), s_sw[r] >> 6, e); };
    if (mask_out) {
        batch_gather<int8_t, kActions, MASK_PITCH>(mask, reinterpret_cast<int8_t *>(s_img), s_prev, L.rows, k, from);
        wave_lds_fence();
        tile_out<kActions, kStoreStream>(mask_out + L.tile * (kTile * kActions), s_img, L.lane, L.rows);
        wave_lds_fence();
    }
    if (visits_out) {
        batch_gather<int16_t, kActions, VISITS_PITCH>(visits, reinterpret_cast<int16_t *>(s_img), s_at, L.rows, k, from);
        wave_lds_fence();
        tile_out<2 * kActions, kStoreStream>(reinterpret_cast<int8_t *>(visits_out) + L.tile * (kTile * 2 * kActions), s_img, L.lane, L.rows);
    }
}

__global__ __launch_bounds__(64) void k_training_batch(BatchArgs A)
{
    __shared__ uint32_t s_img[image_words<kObs>()];
    __shared__ int64_t s_at[kTile], s_prev[kTile];
    __shared__ uint64_t s_inv[kTile];
    __shared__ uint32_t s_sw[kTile];  // swap bits | mover << 6
    Lane L;
    if (!lane_setup(L, A.batch, A.ntiles)) return;
    int64_t at = -1, prev = -1;
    BatchDraw d{0u, 0u, 0};
    if (L.valid) {
        for (uint32_t i = 0; i < (uint32_t)kBatchAttempts && at < 0; ++i) {
            d = batch_draw(A.seed, A.sample_base + (uint64_t)L.b, A.call, i, A.plies, A.n);
            const int64_t c = traj_cell(d.t, d.b, A.ply_stride, A.tile_stride), p = c - A.ply_stride;
            if (batch_valid(A.z, A.done, A.visits, c, p)) { at = c; prev = p; }
        }
    }
    const bool ok = at >= 0;
    const uint32_t code = ok ? d.sym & A.sym_mask : 0u;
    const Sym S = sym_of(code);
    const uint32_t m = ok ? A.mover[at] != 0 : 0u;
    if (L.valid) {
        A.index_out[2 * L.b] = ok ? (int32_t)d.t : -1;  // (two dword stores: index_out is only 4-byte aligned)
        A.index_out[2 * L.b + 1] = ok ? (int32_t)d.b : -1;
        if (A.z_out) A.z_out[L.b] = ok ? A.z[at] : (int8_t)kZOpen;
        if (A.sym_out) A.sym_out[L.b] = (int16_t)code;
    }
    s_at[L.lane] = at; s_prev[L.lane] = prev; s_inv[L.lane] = S.inv; s_sw[L.lane] = S.swaps | (m << 6);
    wave_lds_fence();
    batch_rows<kObs, kActions, kActions>(A.obs, A.mask, A.visits, A.obs_out, A.mask_out, A.visits_out, s_img, s_at, s_prev, s_inv, s_sw, L);
}

// ---- replay buffer (include/gobblet_hip.h, "Replay buffer") -----------------------------------------------------------------------
// gbl_replay_append in three launches, the result a function of the inputs alone (no atomics, no waiting between workgroups):
//   k_replay_count    one wavefront per chunk (the 64 boards of one tile at one ply; chunks in ascending (t, tile) and lanes in ascending
//                     board are the header's order): lane l tests cell l, the chunk's BALLOT goes to the workspace -- the scatter reads
//                     the 8 bytes back instead of the chunk's z, done and visits a second time.
//   k_replay_scan     one workgroup: every thread sums the popcounts of a contiguous stretch of chunks, the workgroup scans the 1 024
//                     sums in LDS, every thread walks its stretch again and leaves each chunk's first rank; the last thread leaves T0
//                     and K for the scatter and writes the new ring_state.
//   k_replay_scatter  one wavefront per chunk: a lane's rank inside the chunk is mbcnt of the ballot; row type after row type the
//                     chunk's source tile comes in as 16-byte vectors (tile_in), the valid rows are closed up and padded to the ring's
//                     pitch in a second LDS image, dword by dword, and leave as whole 16-byte vectors, each to the slot of its row
//                     (the wrap of the ring and the K - capacity cut are per row; no two rows that are written share a slot).
struct ReplayAppendArgs {
    const int8_t *obs, *mask;
    const int16_t *visits;
    const int8_t *z, *done, *mover;
    int8_t *ring_obs;
    int16_t *ring_visits;
    int8_t *ring_meta;
    uint64_t *state, *ws;
    int64_t n, ply_stride, tile_stride, ntiles, chunks;
    uint64_t capacity;
    int32_t tag;
};

constexpr int kReplayScanThreads = 1024;
constexpr int64_t kReplayMaxGrid = (int64_t)1 << 18;  // (more chunks than that: the wavefronts stride over them)

__global__ __launch_bounds__(64) void k_replay_count(ReplayAppendArgs A)
{
    const int lane = threadIdx.x;
    uint64_t *ballots = A.ws + kReplayWsHead;
    for (int64_t c = blockIdx.x; c < A.chunks; c += gridDim.x) {
        const int64_t t = 1 + c / A.ntiles, tile = c % A.ntiles;
        const int64_t at = t * A.ply_stride + tile * A.tile_stride + lane;
        const bool ok = tile * kTile + lane < A.n && batch_valid(A.z, A.done, A.visits, at, at - A.ply_stride);
        const uint64_t votes = __ballot(ok);
        if (lane == 0) ballots[c] = votes;
    }
}

__global__ __launch_bounds__(kReplayScanThreads) void k_replay_scan(ReplayAppendArgs A)
{
    __shared__ uint64_t s_sum[2][kReplayScanThreads];
    const int tid = threadIdx.x;
    const uint64_t *ballots = A.ws + kReplayWsHead;
    uint64_t *bases = A.ws + kReplayWsHead + A.chunks;
    const int64_t per = (A.chunks + kReplayScanThreads - 1) / kReplayScanThreads;
    const int64_t c0 = std::min<int64_t>(tid * per, A.chunks), c1 = std::min<int64_t>(c0 + per, A.chunks);
    uint64_t mine = 0;
    for (int64_t c = c0; c < c1; ++c) mine += (uint64_t)__popcll(ballots[c]);
    s_sum[0][tid] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kReplayScanThreads; d <<= 1) {  // (Hillis-Steele over the two halves of s_sum: one barrier per step)
        s_sum[cur ^ 1][tid] = s_sum[cur][tid] + (tid >= d ? s_sum[cur][tid - d] : 0ull);
        __syncthreads();
        cur ^= 1;
    }
    const uint64_t upto = s_sum[cur][tid];
    uint64_t base = upto - mine;
    for (int64_t c = c0; c < c1; ++c) {
        bases[c] = base;
        base += (uint64_t)__popcll(ballots[c]);
    }
    if (tid == kReplayScanThreads - 1) {
        const uint64_t T0 = A.state[0];
        A.ws[0] = T0; A.ws[1] = upto;
        A.state[0] = T0 + upto; A.state[1] = upto;
    }
}

// close the chunk's valid rows up: dword q of the image `dst` of cnt rows of PITCHB bytes = the bytes of row s_from[q / (PITCHB / 4)] of
// `src` (rows of ROWB bytes, at any byte offset: two dwords and an alignbyte), zeros from byte ROWB on
template <int ROWB, int PITCHB>
__device__ __forceinline__ void replay_pack(const uint32_t *src, uint32_t *dst, const uint8_t *s_from, int cnt, int lane)
{
    constexpr int DW = PITCHB / 4;
    for (int q = lane; q < cnt * DW; q += 64) {
        const int r = q / DW, d = q % DW;
        const int o = (int)s_from[r] * ROWB + 4 * d, left = ROWB - 4 * d;  // (left: bytes of the row from this dword on)
        uint32_t v = 0u;
        if (left > 0) {
            v = __builtin_amdgcn_alignbyte(src[(o >> 2) + 1], src[o >> 2], (uint32_t)o & 3u);  // (the + 1 stays inside the image's slack)
            if (left < 4) v &= (1u << (8 * left)) - 1u;
        }
        dst[q] = v;
    }
}

// the closed-up image out: 16-byte vector q belongs to row q / (PITCHB / 16), which goes to slot s_slot[row] (-1: under the cut)
template <int PITCHB>
__device__ __forceinline__ void replay_store(int8_t *__restrict__ ring, const uint32_t *dst, const int32_t *s_slot, int cnt, int lane)
{
    constexpr int VEC = PITCHB / 16;
    const uint4 *lv = reinterpret_cast<const uint4 *>(dst);
    for (int q = lane; q < cnt * VEC; q += 64) {
        const int32_t slot = s_slot[q / VEC];
        if (slot >= 0) *reinterpret_cast<uint4 *>(ring + (int64_t)slot * PITCHB + (q % VEC) * 16) = lv[q];
    }
}

__global__ __launch_bounds__(64) void k_replay_scatter(ReplayAppendArgs A)
{
    __shared__ uint32_t s_src[image_words<kObs>()];
    __shared__ __attribute__((aligned(16))) uint32_t s_dst[kTile * kReplayObsPitch / 4];
    __shared__ int32_t s_slot[kTile];
    __shared__ uint8_t s_from[kTile];
    const int lane = threadIdx.x;
    const uint64_t *ballots = A.ws + kReplayWsHead, *bases = A.ws + kReplayWsHead + A.chunks;
    const uint64_t T0 = A.ws[0], K = A.ws[1];
    for (int64_t c = blockIdx.x; c < A.chunks; c += gridDim.x) {
        const uint64_t votes = ballots[c];
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)votes), hi = __builtin_amdgcn_readfirstlane((uint32_t)(votes >> 32));
        const int cnt = __popc(lo) + __popc(hi);
        if (cnt == 0) continue;
        const uint64_t R0 = bases[c];
        if (!replay_kept(R0 + (uint64_t)(cnt - 1), K, A.capacity)) continue;  // (the whole chunk lies under the cut)
        const int64_t t = 1 + c / A.ntiles, tile = c % A.ntiles;
        const int64_t left = A.n - tile * kTile, at0 = t * A.ply_stride + tile * A.tile_stride, prev0 = at0 - A.ply_stride;
        const int rows = left < kTile ? (int)left : kTile;
        const bool ok = ((lane < 32 ? lo : hi) >> (lane & 31)) & 1u;
        const int rank = (int)__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
        int8_t z = 0, mv = 0;
        if (ok) {
            z = A.z[at0 + lane];
            mv = (int8_t)(A.mover[at0 + lane] != 0);
            s_from[rank] = (uint8_t)lane;
        }
        if (lane < cnt) {
            const uint64_t R = R0 + (uint64_t)lane;
            s_slot[lane] = replay_kept(R, K, A.capacity) ? (int32_t)replay_slot(T0, R, A.capacity) : -1;
        }
        wave_lds_fence();
        if (A.ring_obs) {
            tile_in<kObs>(A.obs + prev0 * kObs, s_src, lane, rows);
            wave_lds_fence();
            replay_pack<kObs, kReplayObsPitch>(s_src, s_dst, s_from, cnt, lane);
            wave_lds_fence();
            replay_store<kReplayObsPitch>(A.ring_obs, s_dst, s_slot, cnt, lane);
            wave_lds_fence();
        }
        tile_in<2 * kActions>(reinterpret_cast<const int8_t *>(A.visits) + at0 * (2 * kActions), s_src, lane, rows);
        wave_lds_fence();
        replay_pack<2 * kActions, 2 * kReplayVisitsPitch>(s_src, s_dst, s_from, cnt, lane);
        wave_lds_fence();
        replay_store<2 * kReplayVisitsPitch>(reinterpret_cast<int8_t *>(A.ring_visits), s_dst, s_slot, cnt, lane);
        wave_lds_fence();
        tile_in<kActions>(A.mask + prev0 * kActions, s_src, lane, rows);
        wave_lds_fence();
        replay_pack<kActions, kReplayMetaPitch>(s_src, s_dst, s_from, cnt, lane);
        wave_lds_fence();
        if (ok) {  // the row's own scalars, over the zeros the pack left behind the mask
            int8_t *row = reinterpret_cast<int8_t *>(s_dst) + rank * kReplayMetaPitch;
            row[kReplayMetaZ] = z;
            row[kReplayMetaMover] = mv;
            s_dst[(rank * kReplayMetaPitch + kReplayMetaTag) / 4] = (uint32_t)A.tag;
        }
        wave_lds_fence();
        replay_store<kReplayMetaPitch>(A.ring_meta, s_dst, s_slot, cnt, lane);
        wave_lds_fence();  // (the next chunk rebuilds s_from, s_slot and the images)
    }
}

// gbl_replay_batch: k_training_batch with a one-shot phase 1 -- lane l draws sample l's slot from the ring's state (no attempt loop:
// every live row is a sample) and reads the row's z, mover and tag as one 16-byte vector of its meta row -- and the same phases 2 and 3
// (batch_rows) over the ring's pitches: a sample's three source rows are one 128-byte line each (the meta row half of one).
struct ReplayBatchArgs {
    const int8_t *ring_obs;
    const int16_t *ring_visits;
    const int8_t *ring_meta;
    const uint64_t *state;
    int8_t *obs_out, *mask_out;
    int16_t *visits_out;
    int8_t *z_out;
    int32_t *index_out;
    int16_t *sym_out;
    int64_t batch, ntiles, recent;
    uint64_t capacity, seed, sample_base;
    uint32_t call, sym_mask;
};

__global__ __launch_bounds__(64) void k_replay_batch(ReplayBatchArgs A)
{
    __shared__ uint32_t s_img[image_words<kObs>()];
    __shared__ int64_t s_row[kTile];
    __shared__ uint64_t s_inv[kTile];
    __shared__ uint32_t s_sw[kTile];  // swap bits | mover << 6
    Lane L;
    if (!lane_setup(L, A.batch, A.ntiles)) return;
    ReplayDraw d{-1, 0u};
    if (L.valid) d = replay_draw(A.seed, A.sample_base + (uint64_t)L.b, A.call, A.state[0], A.capacity, A.recent);
    const bool ok = d.slot >= 0;
    const uint32_t code = ok ? d.sym & A.sym_mask : 0u;
    const Sym S = sym_of(code);
    uint4 tail{0u, 0u, 0u, 0u};  // bytes 48 .. 63 of the meta row: z and the mover in .y's upper half, the tag in .z
    if (ok) tail = *reinterpret_cast<const uint4 *>(A.ring_meta + d.slot * kReplayMetaPitch + 48);
    const uint32_t m = (tail.y >> 24) != 0u;
    if (L.valid) {
        A.index_out[2 * L.b] = ok ? (int32_t)d.slot : -1;  // (two dword stores: index_out is only 4-byte aligned)
        A.index_out[2 * L.b + 1] = ok ? (int32_t)tail.z : -1;
        if (A.z_out) A.z_out[L.b] = ok ? (int8_t)(tail.y >> 16) : (int8_t)kZOpen;
        if (A.sym_out) A.sym_out[L.b] = (int16_t)code;
    }
    s_row[L.lane] = d.slot; s_inv[L.lane] = S.inv; s_sw[L.lane] = S.swaps | (m << 6);
    wave_lds_fence();
    batch_rows<kReplayObsPitch, kReplayMetaPitch, kReplayVisitsPitch>(A.ring_obs, A.ring_meta, A.ring_visits, A.obs_out, A.mask_out,
                                                                      A.visits_out, s_img, s_row, s_row, s_inv, s_sw, L);
}

// ---- prioritised replay (include/gobblet_hip.h, "Replay buffer", the priorities' paragraph) ------------------------------------------
//   k_replay_prio_append  one wavefront per chunk, as k_replay_scatter: the chunk's ballot and first rank come from the workspace the
//                         append of this window left, a lane's rank is mbcnt of the ballot, and a kept row's priority is one dword store.
//   k_replay_prio_update  PASS 0 stores INT32_MIN to every named slot, PASS 1 applies atomicMax: two launches, so every maximum starts
//                         from INT32_MIN whatever the order of the lanes.
//   k_replay_prio_leaves  one workgroup of 512 threads per block of 64 leaves (8 KB of ring_prio): thread v reads the block's 16-byte vector
//                         v (8 lanes per 128-byte line = leaf), counts only slots that are live, three shuffles leave the leaf's weight
//                         with the line's first lane; the first wavefront scans the 64 weights by shuffles and stores the block's
//                         local prefix and, into base[block + 1], its weight.
//   k_replay_prio_scan    k_replay_scan's form over the blocks' weights, in place: base becomes the exclusive prefix (one block per
//                         thread up to 2^21 slots); the last thread writes the header (the ring_state[0] the index is for, the whole weight).
//   k_replay_batch_prio   k_replay_batch with another phase 1: the span's weight and origin (replay_prio_span: the same scalar work in
//                         every lane, on lines the whole grid shares), then per lane the two binary searches and one leaf, which
//                         comes in as eight independent 16-byte loads (replay_prio_draw).
struct ReplayPrioAppendArgs {
    const int32_t *prio_traj;
    int32_t *ring_prio;
    const uint64_t *ws;
    int64_t ply_stride, tile_stride, ntiles, chunks;
    uint64_t capacity;
    int32_t value;
};

__global__ __launch_bounds__(64) void k_replay_prio_append(ReplayPrioAppendArgs A)
{
    const int lane = threadIdx.x;
    const uint64_t *ballots = A.ws + kReplayWsHead, *bases = A.ws + kReplayWsHead + A.chunks;
    const uint64_t T0 = A.ws[0], K = A.ws[1];
    for (int64_t c = blockIdx.x; c < A.chunks; c += gridDim.x) {
        const uint64_t votes = ballots[c];
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)votes), hi = __builtin_amdgcn_readfirstlane((uint32_t)(votes >> 32));
        const bool ok = ((lane < 32 ? lo : hi) >> (lane & 31)) & 1u;
        if (!ok) continue;
        const uint64_t R = bases[c] + (uint64_t)__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
        if (!replay_kept(R, K, A.capacity)) continue;
        const int64_t at = (1 + c / A.ntiles) * A.ply_stride + (c % A.ntiles) * A.tile_stride + lane;
        A.ring_prio[replay_slot(T0, R, A.capacity)] = A.prio_traj ? A.prio_traj[at] : A.value;
    }
}

template <int PASS>
__global__ __launch_bounds__(256) void k_replay_prio_update(const int32_t *__restrict__ index, const int32_t *__restrict__ values, int64_t batch,
                                                            int32_t *ring_prio, int64_t capacity)
{
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < batch; j += (int64_t)gridDim.x * 256) {
        const int32_t slot = index[2 * j];
        if (slot < 0 || (int64_t)slot >= capacity) continue;
        if (PASS == 0) ring_prio[slot] = INT32_MIN;
        else atomicMax(ring_prio + slot, values[j]);
    }
}

struct ReplayPrioIndexArgs {
    const int32_t *ring_prio;
    const uint64_t *state;
    uint64_t *index;
    uint64_t capacity, leaves, blocks;
};

constexpr int kReplayLeafThreads = kReplayBlockLeaves * 8;  // a 16-byte vector per thread: 8 threads per leaf

__global__ __launch_bounds__(kReplayLeafThreads) void k_replay_prio_leaves(ReplayPrioIndexArgs A)
{
    __shared__ uint64_t s_leaf[kReplayBlockLeaves];
    const int tid = threadIdx.x;
    const uint64_t total = A.state[0], live = total < A.capacity ? total : A.capacity;
    uint64_t *base = A.index + kReplayPrioHead, *local = base + A.blocks + 1u;
    for (uint64_t b = blockIdx.x; b < A.blocks; b += gridDim.x) {
        const uint64_t s = 4u * (b * kReplayLeafThreads + (uint64_t)tid);
        uint64_t sum = 0;
        if (s + 4u <= live) {
            const uint4 p = *reinterpret_cast<const uint4 *>(A.ring_prio + s);
            sum = replay_weight((int32_t)p.x) + replay_weight((int32_t)p.y) + replay_weight((int32_t)p.z) + replay_weight((int32_t)p.w);
        } else {
            for (uint64_t i = s; i < live; ++i) sum += replay_weight(A.ring_prio[i]);  // (the last live vector, dword by dword; none behind it)
        }
        sum += __shfl_xor(sum, 1);
        sum += __shfl_xor(sum, 2);
        sum += __shfl_xor(sum, 4);
        if ((tid & 7) == 0) s_leaf[tid >> 3] = sum;
        __syncthreads();
        if (tid < kReplayBlockLeaves) {  // the first wavefront: an inclusive scan of the 64 weights by shuffles
            const uint64_t mine = s_leaf[tid];
            uint64_t upto = mine;
            for (int d = 1; d < kReplayBlockLeaves; d <<= 1) {
                const uint64_t before = __shfl_up(upto, d);
                if (tid >= d) upto += before;
            }
            const uint64_t leaf = b * kReplayBlockLeaves + (uint64_t)tid;
            if (leaf < A.leaves) local[leaf] = upto - mine;
            if (tid == kReplayBlockLeaves - 1) base[b + 1u] = upto;
        }
        __syncthreads();  // (the next block overwrites s_leaf)
    }
}

__global__ __launch_bounds__(kReplayScanThreads) void k_replay_prio_scan(ReplayPrioIndexArgs A)
{
    __shared__ uint64_t s_sum[2][kReplayScanThreads];
    const int tid = threadIdx.x;
    uint64_t *base = A.index + kReplayPrioHead;
    const uint64_t per = (A.blocks + kReplayScanThreads - 1) / kReplayScanThreads;
    const uint64_t c0 = std::min<uint64_t>(tid * per, A.blocks), c1 = std::min<uint64_t>(c0 + per, A.blocks);
    uint64_t mine = 0;
    for (uint64_t c = c0; c < c1; ++c) mine += base[c + 1];
    s_sum[0][tid] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kReplayScanThreads; d <<= 1) {  // (Hillis-Steele over the two halves of s_sum: one barrier per step)
        s_sum[cur ^ 1][tid] = s_sum[cur][tid] + (tid >= d ? s_sum[cur][tid - d] : 0ull);
        __syncthreads();
        cur ^= 1;
    }
    const uint64_t upto = s_sum[cur][tid];
    uint64_t acc = upto - mine;
    for (uint64_t c = c0; c < c1; ++c) {  // (a block's weight becomes the prefix behind it; base[c0] belongs to the thread before)
        acc += base[c + 1];
        base[c + 1] = acc;
    }
    if (tid == 0) base[0] = 0;
    if (tid == kReplayScanThreads - 1) { A.index[0] = A.state[0]; A.index[1] = upto; }
}

struct ReplayBatchPrioArgs {
    ReplayBatchArgs B;
    const int32_t *ring_prio;
    const uint64_t *index;
    int32_t *prio_out;
    uint64_t *total_out;
};

__global__ __launch_bounds__(64) void k_replay_batch_prio(ReplayBatchPrioArgs P)
{
    __shared__ uint32_t s_img[image_words<kObs>()];
    __shared__ int64_t s_row[kTile];
    __shared__ uint64_t s_inv[kTile];
    __shared__ uint32_t s_sw[kTile];  // swap bits | mover << 6
    const ReplayBatchArgs &A = P.B;
    Lane L;
    if (!lane_setup(L, A.batch, A.ntiles)) return;
    const ReplayPrioSpan span = replay_prio_span(P.ring_prio, P.index, A.state[0], A.capacity, A.recent);
    if (P.total_out && blockIdx.x == 0 && L.lane == 0) { P.total_out[0] = span.W; P.total_out[1] = span.span; }
    ReplayPrioDraw d{-1, 0u, 0u};
    if (L.valid) d = replay_prio_draw(A.seed, A.sample_base + (uint64_t)L.b, A.call, span, A.capacity, P.ring_prio, P.index);
    const bool ok = d.slot >= 0;
    const uint32_t code = ok ? d.sym & A.sym_mask : 0u;
    const Sym S = sym_of(code);
    uint4 tail{0u, 0u, 0u, 0u};  // bytes 48 .. 63 of the meta row: z and the mover in .y's upper half, the tag in .z
    if (ok) tail = *reinterpret_cast<const uint4 *>(A.ring_meta + d.slot * kReplayMetaPitch + 48);
    const uint32_t m = (tail.y >> 24) != 0u;
    if (L.valid) {
        A.index_out[2 * L.b] = ok ? (int32_t)d.slot : -1;  // (two dword stores: index_out is only 4-byte aligned)
        A.index_out[2 * L.b + 1] = ok ? (int32_t)tail.z : -1;
        if (P.prio_out) P.prio_out[L.b] = (int32_t)d.weight;
        if (A.z_out) A.z_out[L.b] = ok ? (int8_t)(tail.y >> 16) : (int8_t)kZOpen;
        if (A.sym_out) A.sym_out[L.b] = (int16_t)code;
    }
    s_row[L.lane] = d.slot; s_inv[L.lane] = S.inv; s_sw[L.lane] = S.swaps | (m << 6);
    wave_lds_fence();
    batch_rows<kReplayObsPitch, kReplayMetaPitch, kReplayVisitsPitch>(A.ring_obs, A.ring_meta, A.ring_visits, A.obs_out, A.mask_out,
                                                                      A.visits_out, s_img, s_row, s_row, s_inv, s_sw, L);
}

// ---- tablebase (include/gobblet_hip.h, "Exact tablebase") ---------------------------------------------------------------------------
// k_tb_prepare   one workgroup fills `aux`: every thread classifies a stretch of the 19 683 ternary level numbers, the workgroup scans
//                the counts (both rank tables at once, packed into one word), every thread writes its stretch's ranks and inverses.
// k_tb_sweep     one lane per position, grid-stride; the whole of `aux` (61.6 KB) in LDS, loaded once per workgroup.  A lane whose byte
//                is already decided does nothing; the others walk their moves (tb_sweep_value): integer work that diverges from lane to
//                lane and one byte load per quiet move from anywhere in the table.  Only bytes that change are stored.  The count of
//                stores goes out as one atomic per wavefront.  Indices are below 2^32; the range counter and every offset are 64-bit.
// k_tb_probe     one wavefront per board, lane a < 54 per action (board_planes / board_candidates as k_solve); the three look-ups of
//                an action's successor go to `aux` in global memory (a board is too little work to stage 61.6 KB for).
// k_tb_index / k_tb_position   one lane per board.
constexpr int kTbThreads = 1024;
constexpr int kTbSweepGroups = 512;
constexpr int kTbPrepareSpan = (kTbTernary + kTbThreads - 1) / kTbThreads;  // level numbers per thread of k_tb_prepare

__global__ __launch_bounds__(kTbThreads) void k_tb_prepare(uint8_t *aux)
{
    __shared__ uint32_t s_sum[2][kTbThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = std::min(tid * (uint32_t)kTbPrepareSpan, kTbTernary), t1 = std::min(t0 + (uint32_t)kTbPrepareSpan, kTbTernary);
    uint32_t mine = 0;
    for (uint32_t t = t0; t < t1; ++t) mine += tb_admissible(t);
    s_sum[0][tid] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kTbThreads; d <<= 1) {  // (Hillis-Steele over the two halves of s_sum, as k_replay_scan; neither half-word carries: 1 423 and 91)
        s_sum[cur ^ 1][tid] = s_sum[cur][tid] + (tid >= (uint32_t)d ? s_sum[cur][tid - d] : 0u);
        __syncthreads();
        cur ^= 1;
    }
    uint32_t base = s_sum[cur][tid] - mine;
    uint16_t *rank2 = reinterpret_cast<uint16_t *>(aux + kTbAuxRank2), *inv2 = reinterpret_cast<uint16_t *>(aux + kTbAuxInv2),
             *inv1 = reinterpret_cast<uint16_t *>(aux + kTbAuxInv1), *tern = reinterpret_cast<uint16_t *>(aux + kTbAuxTern);
    uint8_t *rank1 = aux + kTbAuxRank1;
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t f = tb_admissible(t), r2 = base & 0xFFFFu, r1 = base >> 16;
        rank2[t] = (f & 1u) ? (uint16_t)r2 : (uint16_t)0xFFFFu;
        rank1[t] = (f >> 16) ? (uint8_t)r1 : (uint8_t)0xFFu;
        if (f & 1u) inv2[r2] = (uint16_t)t;
        if (f >> 16) inv1[r1] = (uint16_t)t;
        base += f;
    }
    if (tid < 512u) tern[tid] = (uint16_t)tb_tern_of(tid);
    // the padding between the tables, so that `aux` is comparable byte for byte
    if (tid == 0) {
        rank2[kTbTernary] = 0; inv2[kTbLevels2] = 0; inv1[kTbLevels1] = 0;
        for (uint32_t i = kTbAuxRank1 + kTbTernary; i < kTbAuxBytes; ++i) aux[i] = 0;
    }
}

struct TbSweepArgs {
    const uint32_t *aux;
    const int8_t *table;
    int8_t *out;  // (may alias table: no __restrict__ on either)
    unsigned long long *decided;
    uint64_t first, count;
    TbShape S;
    int k;
};

__global__ __launch_bounds__(kTbThreads) void k_tb_sweep(TbSweepArgs a)
{
    __shared__ uint32_t s_aux[kTbAuxBytes / 4];
    for (uint32_t i = threadIdx.x; i < kTbAuxBytes / 4; i += kTbThreads) s_aux[i] = a.aux[i];
    __syncthreads();
    const TbAux A = tb_aux(s_aux);
    const uint64_t step = (uint64_t)gridDim.x * kTbThreads;
    uint32_t wrote = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kTbThreads + threadIdx.x; j < a.count; j += step) {
        if (a.k > 0 && a.out[j] != 0) continue;
        const TbPos p = tb_position_of(A, a.S, (uint32_t)(a.first + j));
        if (a.k == 0) {
            const int v = tb_winner(p.own, p.oth) != 0 ? kTbTerminal : 0;
            a.out[j] = (int8_t)v;
            wrote += v != 0;
        } else {
            const int v = tb_sweep_value(A, a.S, p, a.k, a.table);
            if (v == a.k || v == -a.k) {
                a.out[j] = (int8_t)v;
                ++wrote;
            }
        }
    }
    const uint32_t sum = wave_sum(wrote);
    if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(a.decided, (unsigned long long)sum);
}

__global__ __launch_bounds__(64) void k_tb_probe(const uint8_t *__restrict__ aux, const int8_t *__restrict__ table, const int8_t *__restrict__ state,
                                                 const int8_t *__restrict__ to_move, const int8_t *__restrict__ mask,
                                                 int8_t *__restrict__ outcome_out, int8_t *__restrict__ value_out, int32_t *__restrict__ action_out,
                                                 int64_t n, TbShape S)
{
    const TbAux A = tb_aux(aux);
    const uint32_t lane = threadIdx.x;
    const uint64_t pieces = tb_piece_actions(S);
    for (int64_t b = blockIdx.x; b < n; b += gridDim.x) {
        const Planes root = board_planes(state, b, lane);
        const int mover = to_move[b] != 0;
        uint64_t cand = board_candidates(root, mover, mask, b, lane) & pieces;
        if (tb_board_index(A, S, root, mover) < 0) cand = 0;
        const bool mine = lane < (uint32_t)kActions && ((cand >> lane) & 1ull);
        const int c = mine ? tb_probe_action(A, S, table, root, mover, lane) : kSolveNone;
        const uint32_t best = wave_max(mine ? tb_action_key(c, lane) : 0u);
        if (outcome_out && lane < (uint32_t)kActions) outcome_out[b * kActions + lane] = (int8_t)c;
        if (lane == 0) {
            if (value_out) value_out[b] = (int8_t)tb_value_of(best);
            if (action_out) action_out[b] = tb_action_of(best);
        }
    }
}

__global__ __launch_bounds__(256) void k_tb_index(const uint8_t *__restrict__ aux, const int8_t *__restrict__ state, const int8_t *__restrict__ to_move,
                                                  int64_t *__restrict__ index_out, int64_t n, TbShape S)
{
    const TbAux A = tb_aux(aux);
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < n; b += (int64_t)gridDim.x * 256) {
        Planes p{0u, 0u, 0u};
        for (int cell = 0; cell < kCells; ++cell) {
            const int v = state[b * kCells + cell];
            p.nz |= (uint32_t)(v != 0) << cell;
            p.neg |= (uint32_t)(v < 0) << cell;
            p.odd |= (uint32_t)(v & 1) << cell;
        }
        index_out[b] = tb_board_index(A, S, p, to_move[b] != 0);
    }
}

__global__ __launch_bounds__(256) void k_tb_position(const uint8_t *__restrict__ aux, const int64_t *__restrict__ index, int8_t *__restrict__ state_out,
                                                     int64_t n, TbShape S)
{
    const TbAux A = tb_aux(aux);
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < n; b += (int64_t)gridDim.x * 256) tb_row_of(A, S, index[b], state_out + b * kCells);
}

// ---- tablebase targets (include/gobblet_hip.h, "Tablebase targets") -------------------------------------------------------------------
// k_tb_targets   one wavefront per row (four per workgroup, rows dealt grid-stride), lane a < 54 per action, as k_tb_probe.  The board
//                never exists as a state row: lane c < 27 reads the four observation bytes that make cell c (two pairs of neighbours),
//                lanes 27 .. 35 the nine agent bytes, and five ballots are the mover and the planes (decode_obs_row's arithmetic per
//                cell, so any 117 bytes decode alike).  The byte loads go to at most two lines of the row; nothing is staged in LDS.
//                R, S, the old visits' argmax and the census are ballots and butterfly reductions.  Every row is read (its old z and
//                visits too) before any of its bytes is written, so visits_out / z_out may be visits_in / z_in.
constexpr int kTbTargetWaves = 4;
constexpr int kTbTargetGroups = 4096;  // the grid's cap: 16 384 rows in flight, the rest by the stride

struct TbTargetArgs {
    const uint8_t *aux;
    const int8_t *table, *obs, *mask;
    const int16_t *visits_in;  // (may be visits_out, and z_in z_out: no __restrict__ anywhere here)
    int16_t *visits_out;
    const int8_t *z_in;
    int8_t *z_out, *value_out, *outcome_out, *census_out;
    int64_t obs_pitch, mask_pitch, visits_pitch, z_pitch, n;
    TbShape S;
    int mode, count;
};

// the planes and the mover of one observation row, in every lane
__device__ __forceinline__ Planes obs_planes(const int8_t *o, uint32_t lane, int &mover)
{
    int v = 0, agent = 0;
    if (lane < (uint32_t)kCells) {
        const uint32_t k = (lane * 57u) >> 9, q = lane - 9u * k;  // (lane / 9 for lane < 64)
        const int8_t *c = o + 13u * q + 2u * k;
        const int lo = 2 * (int)k + 1;
        const int bp = lo * c[0] + (lo + 1) * c[1], bo = lo * c[6] + (lo + 1) * c[7];  // greedy_policy.py:44-56
        v = bp > bo ? bp : -bo;                                                      // :57
    } else if (lane < (uint32_t)kCells + 9u) {
        agent = o[13u * (lane - (uint32_t)kCells) + 12u];
    }
    const uint64_t one = __ballot(agent > 0), more = __ballot(agent > 1);  // obs[..., 12].max() over 0: > 0 moves second, == 1 negates (:67-68)
    mover = one != 0ull;
    if (one != 0ull && more == 0ull) v = -v;
    return Planes{(uint32_t)__ballot((v & 0xFF) != 0), (uint32_t)__ballot((v & 0x80) != 0), (uint32_t)__ballot(v & 1)};
}

__global__ __launch_bounds__(64 * kTbTargetWaves) void k_tb_targets(TbTargetArgs a)
{
    const TbAux A = tb_aux(a.aux);
    const uint32_t lane = threadIdx.x & 63u;
    const bool act = lane < (uint32_t)kActions;
    const uint64_t pieces = tb_piece_actions(a.S);
    const int64_t step = (int64_t)gridDim.x * kTbTargetWaves;
    for (int64_t r = (int64_t)blockIdx.x * kTbTargetWaves + uniform((int)(threadIdx.x >> 6)); r < a.n; r += step) {
        const int z_old = a.z_in ? uniform((int)a.z_in[r * a.z_pitch]) : 0;
        int c = kSolveNone, value = 0, census = -1;
        if (!(a.z_in && z_old == kZOpen)) {  // (uniform) a skipped row writes neither visits nor z
            int mover;
            const Planes root = obs_planes(a.obs + r * a.obs_pitch, lane, mover);
            uint64_t cand = board_candidates(root, mover, a.mask ? a.mask + r * a.mask_pitch : nullptr, 0, lane) & pieces;
            if (tb_board_index(A, a.S, root, mover) < 0) cand = 0;
            const bool mine = act && ((cand >> lane) & 1ull);
            if (mine) c = (int)(int8_t)tb_probe_action(A, a.S, a.table, root, mover, lane);  // (the outcome byte: see tb_target_keeps)
            const uint32_t best = wave_max(mine ? tb_action_key(c, lane) : 0u);
            value = tb_value_of(best);
            const int sign = tb_sign(value);
            if (a.census_out && best) {
                const int old = a.visits_in && act ? (int)a.visits_in[r * a.visits_pitch + lane] : 0;
                const uint32_t top = wave_max(tb_visit_key(old, lane));
                census = tb_census(top, __ballot(mine && tb_target_keeps(c, value, kTbTargetResult)), a.z_in != nullptr, z_old, sign);
            }
            if (a.visits_out && act) a.visits_out[r * a.visits_pitch + lane] = (int16_t)(best && mine && tb_target_keeps(c, value, a.mode) ? a.count : 0);
            if (lane == 0) a.z_out[r * a.z_pitch] = (int8_t)(best ? sign : kZOpen);
        }
        if (a.outcome_out && act) a.outcome_out[r * kActions + lane] = (int8_t)c;
        if (lane == 0) {
            if (a.value_out) a.value_out[r] = (int8_t)value;
            if (a.census_out) a.census_out[r] = (int8_t)census;
        }
    }
}

// ---- reanalysis (include/gobblet_hip.h, "Reanalysis") ---------------------------------------------------------------------------------
// k_reanalyse    k_tree_eval's geometry over pitched rows: one wavefront per row, one wavefront per workgroup, a grid-stride loop over the
//                rows, the tree in (iterations + 1) 16-byte nodes and 56-byte prior rows of dynamic LDS beside s_h.  The board never
//                exists as a state row (obs_planes, as k_tb_targets); the search is tree_eval_iterations<false>, the code k_tree_eval
//                and k_collect_eval run.  Lane a then holds the root's child of action a (tree_lane_child): the decision, the two
//                argmaxes and the sums So, Sn and sum |o_a Sn - n_a So| are butterflies, the division is one per row.  The old visits
//                are read before the new ones are stored, so visits_out may be visits_in.
struct ReanalyseArgs {
    EvalNet net;
    const int8_t *obs, *mask;
    const int16_t *visits_in;  // (may be visits_out: no __restrict__ here)
    int16_t *visits_out;
    const int8_t *z_in;
    int32_t *root_value_out;
    uint8_t *root_priors_out;
    int32_t *action_out, *nodes_out, *drift_out;
    int8_t *census_out;
    int64_t obs_pitch, mask_pitch, visits_pitch, z_pitch, n;
    uint32_t iterations, explore;
};

// GUMBEL: gbl_reanalyse_gumbel -- the root follows the Gumbel rule (tree_eval_iterations<false, true>, board id env_base + r), the
// decision and the row's new bytes come from wave_gumbel_finish on the same read-out: lane a stores its target byte where the other form
// stores its child's visits.  Sn can now reach 54 * 255, so the sum of the |o_a Sn - n_a So| (each still below 2^29) is taken in two
// 16-bit halves and the drift in 64 bits (reanalyse_drift64); nothing else differs.  The other form's arguments stay as they were.
struct ReanalyseGumbelArgs : ReanalyseArgs {
    GumbelArgs G;
    uint64_t seed, env_base;
    uint32_t call;
    int16_t *gumbel_out;
};

template <bool GUMBEL>
__global__ __launch_bounds__(64) void k_reanalyse(const std::conditional_t<GUMBEL, ReanalyseGumbelArgs, ReanalyseArgs> a)
{
    extern __shared__ uint4 s_tree[];
    TreeNode *const nodes = reinterpret_cast<TreeNode *>(s_tree);
    uint8_t *const pri = reinterpret_cast<uint8_t *>(nodes + a.iterations + 1);
    __shared__ uint32_t s_h[kEvalMaxHidden / 4];
    const uint32_t lane = threadIdx.x;
    const bool act = lane < (uint32_t)kActions;
    for (int64_t r = blockIdx.x; r < a.n; r += gridDim.x) {
        const int z_old = a.z_in ? uniform((int)a.z_in[r * a.z_pitch]) : 0;
        int q = 0, action = -1, drift = -1, census = -1;
        [[maybe_unused]] int gum = 0;
        uint32_t count = 0, pi = 0;
        if (!(a.z_in && z_old == kZOpen)) {  // (uniform) a skipped row writes no visits
            int mover;
            const Planes root = obs_planes(a.obs + r * a.obs_pitch, lane, mover);
            const uint64_t cand = board_candidates(root, mover, a.mask ? a.mask + r * a.mask_pitch : nullptr, 0, lane);
            uint32_t mixed, now;
            WaveEval at_root;
            if constexpr (GUMBEL) {
                WaveGumbel gb{a.G, a.seed, a.env_base + (uint64_t)r, a.call, 0, 0, 0ull};
                at_root = tree_eval_iterations<false, true>(nodes, pri, s_h, a.net, root, mover, cand, a.iterations, a.explore, lane, count,
                                                            RootNoise{}, mixed, &gb);
                const GumbelOut out = wave_gumbel_out(gb, nodes, cand, at_root.q, lane);
                now = out.target;
                action = out.action;
                gum = gb.gum;
            } else {
                at_root = tree_eval_iterations<false>(nodes, pri, s_h, a.net, root, mover, cand, a.iterations, a.explore, lane, count, RootNoise{},
                                                      mixed);
                const TreeChild c = tree_lane_child(nodes, nodes[0].child, lane);
                now = c.visits();
                action = tree_action_of(wave_max(c.mine() ? tree_final_key(c.n, c.w, c.l, lane) : 0ull));
            }
            q = at_root.q;
            pi = at_root.pi;
            if (cand && (a.drift_out || a.census_out)) {  // (uniform)
                const uint32_t old = a.visits_in && act ? (uint32_t)max((int)a.visits_in[r * a.visits_pitch + lane], 0) : 0u;
                const uint32_t So = wave_sum(old), Sn = wave_sum(now);
                if (a.drift_out) {
                    const uint32_t x = old * Sn, y = now * So, d = x > y ? x - y : y - x;
                    if constexpr (GUMBEL)
                        drift = reanalyse_drift64(a.visits_in != nullptr, So, Sn, ((uint64_t)wave_sum(d >> 16) << 16) + wave_sum(d & 0xFFFFu));
                    else
                        drift = reanalyse_drift(a.visits_in != nullptr, So, Sn, wave_sum(d));
                }
                if (a.census_out)
                    census = reanalyse_census(wave_max(tb_visit_key((int)old, lane)), wave_max(tb_visit_key((int)now, lane)), a.z_in != nullptr,
                                              z_old, q);
            }
            if (a.visits_out && act) a.visits_out[r * a.visits_pitch + lane] = (int16_t)now;
            wave_lds_fence();  // (before the next row rewrites the root)
        }
        if (a.root_priors_out && act) a.root_priors_out[r * kActions + lane] = (uint8_t)pi;
        if constexpr (GUMBEL)
            if (a.gumbel_out && act) a.gumbel_out[r * kActions + lane] = (int16_t)gum;
        if (lane == 0) {
            if (a.root_value_out) a.root_value_out[r] = q;
            if (a.action_out) a.action_out[r] = action;
            if (a.nodes_out) a.nodes_out[r] = (int32_t)count;
            if (a.drift_out) a.drift_out[r] = drift;
            if (a.census_out) a.census_out[r] = (int8_t)census;
        }
    }
}

// gbl_train_step: the float trainer's Adam step in two launches, bit-defined by the header (every float operation below is the
// header's, in its order; GBL_FP_STRICT keeps hipcc from fusing them).
//   k_train_rows          one wavefront per row (four per workgroup, rows dealt grid-stride), w2 staged in LDS once per workgroup:
//                         forward, softmax, losses, do and dh of the row, left in the workspace.
//   k_train_reduce_adam   64 parameter elements per workgroup, one per lane; its 16 wavefronts take the 64-row chunks round robin,
//                         wavefront 0 adds the chunk sums in ascending order, forms g and applies Adam.  The last workgroup's spare
//                         lanes reduce the loss terms and the hidden maximum for stats_out.
struct TrainArgs {
    const int8_t *obs, *mask;
    const int16_t *visits;
    const int8_t *z;
    float *params, *adam_m, *adam_v, *grad_out, *stats_out;
    float *ws_h, *ws_dh, *ws_do, *ws_row;
    int64_t batch;
    int hidden;
    TrainHyper hy;
};

constexpr int kTrainRowWaves = 4;                       // wavefronts (rows in flight) per workgroup of k_train_rows
constexpr int kTrainRowScratch = 4 * kTrainDoStride;    // per wavefront beside h: o, e, the loss terms, do
constexpr int kTrainReduceWaves = 16;

inline size_t train_rows_lds(int hidden)
{
    return sizeof(float) * ((size_t)hidden * kTrainOutputs + kTrainRowWaves * ((size_t)hidden + kTrainRowScratch));
}

// the set bits of a wavefront-uniform mask in ascending order
template <typename F>
__device__ __forceinline__ void each_bit(uint64_t bits, F f)
{
    while (bits) {
        f(__builtin_ctzll(bits));
        bits &= bits - 1;
    }
}

// gbl_train_step_weighted's rows kernel takes the step's arguments and, behind them, the rows' weights and the two per-row outputs
struct TrainExArgs : TrainArgs {
    const float *row_weight;
    float *row_loss_out;
    int32_t *prio_out;
    float prio_scale;
    int32_t prio_floor, prio_cap;
};

// EX = false: gbl_train_step's kernel.  EX = true: gbl_train_step_weighted's -- the row's weight ww, wavefront-uniform and held in a scalar
// register, is folded into the stores of do and of the loss terms, and the lanes that hold lp and lv write the two per-row outputs
// (EX asks the compiler for 4 / 4 / 2 / 2 wavefronts per SIMD by name: without that <2, true> lands at 131 VGPRs, just past the step
// from 4 to 3.  <3, true> does not fit gbl_train_step's 168 -- asked for 3 wavefronts it spills two registers -- and runs 2 per SIMD)
template <int U, bool EX = false>  // U = H / 64: hidden units per lane
__global__ __launch_bounds__(64 * kTrainRowWaves) __attribute__((amdgpu_waves_per_eu(EX ? (U <= 2 ? 4 : 2) : 1)))
void k_train_rows(std::conditional_t<EX, TrainExArgs, TrainArgs> A)
{
    GBL_FP_STRICT
    constexpr int H = 64 * U;
    extern __shared__ __align__(16) float s_train[];  // w2 [H][55]; then per wavefront h [H], o / e / terms / do [56] each
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float *w2s = s_train;
    float *sh = s_train + H * kTrainOutputs + wave * (H + kTrainRowScratch);
    float *so = sh + H, *se = so + kTrainDoStride, *st = se + kTrainDoStride, *sd = st + kTrainDoStride;
    const float *__restrict__ w1 = A.params, *__restrict__ b1 = w1 + kObs * H, *__restrict__ w2 = b1 + H,
                *__restrict__ b2 = w2 + H * kTrainOutputs;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(H * kTrainOutputs); i += 64u * kTrainRowWaves) w2s[i] = w2[i];
    __syncthreads();  // (the only rendezvous: from here the wavefronts share nothing but the read-only w2)
    for (int64_t r = (int64_t)blockIdx.x * kTrainRowWaves + wave; r < A.batch; r += (int64_t)gridDim.x * kTrainRowWaves) {
        float *rh = A.ws_h + r * H, *rdh = A.ws_dh + r * H, *rdo = A.ws_do + r * kTrainDoStride, *rst = A.ws_row + r * kTrainRowStats;
        // (EX: the row as a scalar -- r < 2^16 --, so that the addresses of the row's weight and of its two outputs cost no vector registers)
        const int64_t rs = EX ? (int64_t)__builtin_amdgcn_readfirstlane((int)r) : r;
        const bool action = lane < (uint32_t)kActions;
        const bool in_c = action && (!A.mask || A.mask[r * kActions + lane] != 0);
        const uint64_t cand = __ballot(in_c);
        const int vis = in_c ? (int)A.visits[r * kActions + lane] : 0;
        const int S = (int)wave_sum((uint32_t)vis);
        const int z = A.z[r];
        if (z == kZOpen || S <= 0) {  // (uniform) an uncounted row: zeros everywhere
#pragma unroll
            for (int u = 0; u < U; ++u) rh[lane + 64 * u] = rdh[lane + 64 * u] = 0.0f;
            if (lane < (uint32_t)kTrainDoStride) rdo[lane] = 0.0f;
            if (lane < (uint32_t)kTrainRowStats) rst[lane] = 0.0f;
            if constexpr (EX) {
                if (A.row_loss_out && lane < 2u) A.row_loss_out[2 * rs + lane] = 0.0f;
                if (A.prio_out && lane == 0u) A.prio_out[rs] = 0;
            }
            continue;
        }
        float ww = 1.0f;  // (uniform: one scalar load per row)
        if constexpr (EX) {
            if (A.row_weight)
                ww = train_bits_float(train_weight_bits((uint32_t)__builtin_amdgcn_readfirstlane((int)train_float_bits(A.row_weight[rs]))));
        }
        // layer 1: the w1 rows of the set bytes, ascending
        const uint64_t set0 = __ballot(A.obs[r * kObs + lane] != 0);
        const uint64_t set1 = __ballot(lane + 64u < (uint32_t)kObs && A.obs[r * kObs + (lane + 64u < (uint32_t)kObs ? lane + 64u : 0u)] != 0);
        float pre[U];
#pragma unroll
        for (int u = 0; u < U; ++u) pre[u] = b1[lane + 64 * u];
        each_bit(set0, [&](int f) {
#pragma unroll
            for (int u = 0; u < U; ++u) pre[u] = pre[u] + w1[f * H + lane + 64 * u];
        });
        each_bit(set1, [&](int f) {
#pragma unroll
            for (int u = 0; u < U; ++u) pre[u] = pre[u] + w1[(f + 64) * H + lane + 64 * u];
        });
        uint32_t top = 0u;  // (the bits of non-negative floats order as the floats do)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float h = pre[u] > 0.0f ? pre[u] : 0.0f;
            sh[lane + 64 * u] = rh[lane + 64 * u] = h;
            top = train_float_bits(h) > top ? train_float_bits(h) : top;
        }
        top = wave_max(top);
        wave_lds_fence();
        // layer 2: lane k owns o_k
        float o = 0.0f;
        if (lane < (uint32_t)kTrainOutputs) {
            o = b2[lane];
            for (int j = 0; j < H; ++j) o = o + sh[j] * w2s[j * kTrainOutputs + lane];
        }
        if (lane < (uint32_t)kTrainDoStride) so[lane] = o;
        wave_lds_fence();
        // the softmax over C: every lane walks the candidates in ascending order (the sums have ONE order), lane a keeps its own e_a
        float mx = so[__builtin_ctzll(cand)];
        each_bit(cand & (cand - 1), [&](int a) {
            const float v = so[a];
            mx = v > mx ? v : mx;
        });
        const float d = o - mx;
        const float e = in_c ? train_exp(d) : 0.0f;
        if (lane < (uint32_t)kTrainDoStride) se[lane] = e;
        wave_lds_fence();
        float s = 0.0f;
        each_bit(cand, [&](int a) { s = s + se[a]; });
        const float L = train_log(s);
        float g = 0.0f, term = 0.0f, lv = 0.0f;
        if (in_c) train_policy(e, s, d, L, vis, S, g, term);
        if (lane == (uint32_t)kActions) train_value(o, z, A.hy.value_reg, lv, g);
        if (lane < (uint32_t)kTrainDoStride) {
            st[lane] = term;
            sd[lane] = EX ? ww * g : g;
            rdo[lane] = EX ? ww * g : g;
        }
        wave_lds_fence();
        float lp = 0.0f;
        each_bit(cand, [&](int a) { lp = lp + st[a]; });
        if (lane == 0u) {
            rst[0] = EX ? ww * lp : lp;
            rst[2] = train_bits_float(top);
            rst[3] = 1.0f;
        }
        if (lane == (uint32_t)kActions) rst[1] = EX ? ww * lv : lv;
        if constexpr (EX) {  // the unweighted loss terms, from the lanes that hold them: lane 0 has lp, lane 54 has lp and lv
            if (A.row_loss_out && lane == 0u) A.row_loss_out[2 * rs] = lp;
            if (A.row_loss_out && lane == (uint32_t)kActions) A.row_loss_out[2 * rs + 1] = lv;
            if (A.prio_out && lane == (uint32_t)kActions) A.prio_out[rs] = train_priority(lp, lv, A.prio_scale, A.prio_floor, A.prio_cap);
        }
        // backward through layer 2: lane j owns dh_j
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = (int)lane + 64 * u;
            float acc = 0.0f;
            for (int k = 0; k < kTrainOutputs; ++k) acc = acc + sd[k] * w2s[j * kTrainOutputs + k];
            rdh[j] = pre[u] > 0.0f ? acc : 0.0f;
        }
        wave_lds_fence();  // (every lane has read this row's LDS before the next row overwrites it)
    }
}

// rows [r0, r1) of one chunk, ascending, for the lane's element.  KIND 0: an element of w1 (x points at the rows' byte f);
// 1: a plain column (b1, b2, the loss terms); 2: an element of w2 (a product of two columns)
template <int KIND>
__device__ __forceinline__ float train_chunk_sum(const float *__restrict__ a, int64_t stride_a, const float *__restrict__ b,
                                                 const int8_t *__restrict__ x, int64_t r0, int64_t r1)
{
    GBL_FP_STRICT
    float acc = 0.0f;
#pragma unroll 8
    for (int64_t r = r0; r < r1; ++r) {
        if (KIND == 0) {
            if (x[r * kObs] != 0) acc = acc + a[r * stride_a];
        } else if (KIND == 1) {
            acc = acc + a[r * stride_a];
        } else {
            acc = acc + a[r * stride_a] * b[r * kTrainDoStride];
        }
    }
    return acc;
}

// the larger of two non-negative floats, on their bits (which order as the floats do)
__device__ __forceinline__ float train_max(float a, float b) { return train_float_bits(b) > train_float_bits(a) ? b : a; }

__global__ __launch_bounds__(64 * kTrainReduceWaves) void k_train_reduce_adam(TrainArgs A)
{
    GBL_FP_STRICT
    __shared__ float s_part[kTrainReduceWaves][64];
    __shared__ int s_count[kTrainReduceWaves];
    const int H = A.hidden, P = train_param_count(H);
    const int64_t B = A.batch;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int first = (int)blockIdx.x * 64, e = first + (int)lane;  // this workgroup's elements; first is a multiple of 64
    // N, the counted rows (an integer count: any order)
    int mine = 0;
    for (int64_t r = threadIdx.x; r < B; r += 64 * kTrainReduceWaves) mine += A.ws_row[r * kTrainRowStats + 3] != 0.0f;
    mine = (int)wave_sum((uint32_t)mine);
    if (lane == 0u) s_count[wave] = mine;
    __syncthreads();
    int N = 0;
#pragma unroll
    for (int w = 0; w < kTrainReduceWaves; ++w) N += s_count[w];
    // what this lane sums.  The regions w1 / b1 / w2 begin at multiples of 64 elements (H is one), so a workgroup lies in ONE
    // region -- except the last, which holds b2 and, in its spare lanes, the two loss terms and the hidden maximum
    const int at_b1 = kObs * H, at_w2 = at_b1 + H, at_b2 = at_w2 + kTrainOutputs * H;
    const int region = first < at_b1 ? 0 : first < at_w2 ? 1 : first < at_b2 ? 2 : 3;  // (uniform)
    const float *a = A.ws_row, *b = A.ws_do;
    const int8_t *x = A.obs;
    int64_t stride = 0;  // (a spare lane past the statistics sums the first row's lp with stride 0 and drops it)
    if (region == 0) {
        const int f = first / H;
        x = A.obs + f; a = A.ws_dh + (e - f * H); stride = H;
    } else if (region == 1) {
        a = A.ws_dh + (e - at_b1); stride = H;
    } else if (region == 2) {
        const int j = (e - at_w2) / kTrainOutputs, k = (e - at_w2) - j * kTrainOutputs;
        a = A.ws_h + j; b = A.ws_do + k; stride = H;
    } else if (e < P) {
        a = A.ws_do + (e - at_b2); stride = kTrainDoStride;
    } else if (e < P + 3) {
        a = A.ws_row + (e - P); stride = kTrainRowStats;
    }
    const bool is_max = e == P + 2;
    const int64_t chunks = (B + kTrainChunk - 1) / kTrainChunk;
    float total = 0.0f;
    for (int64_t c0 = 0; c0 < chunks; c0 += kTrainReduceWaves) {
        const int64_t c = c0 + wave, r0 = c * kTrainChunk, r1 = r0 + kTrainChunk < B ? r0 + kTrainChunk : B;
        float acc = 0.0f;
        if (c < chunks) {
            if (region == 0) acc = train_chunk_sum<0>(a, stride, b, x, r0, r1);
            else if (region == 1) acc = train_chunk_sum<1>(a, stride, b, x, r0, r1);
            else if (region == 2) acc = train_chunk_sum<2>(a, stride, b, x, r0, r1);
            else if (!is_max) acc = train_chunk_sum<1>(a, stride, b, x, r0, r1);
            else
                for (int64_t r = r0; r < r1; ++r) acc = train_max(acc, a[r * stride]);
        }
        s_part[wave][lane] = acc;
        __syncthreads();
        if (wave == 0u) {
            const int live = chunks - c0 < kTrainReduceWaves ? (int)(chunks - c0) : kTrainReduceWaves;
            for (int w = 0; w < live; ++w) {
                const float p = s_part[w][lane];
                total = is_max ? train_max(total, p) : total + p;
            }
        }
        __syncthreads();  // (wavefront 0 has read the chunk sums before the next round overwrites them)
    }
    if (wave != 0u) return;
    const float M = (float)(N > 0 ? N : 1);
    if (e < P) {
        float theta = A.params[e], m = A.adam_m[e], v = A.adam_v[e];
        const float g = train_gradient(total, M, theta, A.hy);
        train_adam(g, theta, m, v, A.hy);
        A.params[e] = theta; A.adam_m[e] = m; A.adam_v[e] = v;
        if (A.grad_out) A.grad_out[e] = g;
    } else if (e < P + 2) {
        A.stats_out[e - P] = total / M;
    } else if (is_max) {
        A.stats_out[2] = (float)N;
        A.stats_out[3] = total;
    }
}

// gbl_replay_importance: one launch, every workgroup finds the batch's smallest positive priority itself (an integer minimum over an
// array of at most 256 KB that stays in L2: any order), then weighs its own 256 entries.  No atomics, no waiting between workgroups.
constexpr int kImportanceThreads = 256;

__global__ __launch_bounds__(kImportanceThreads) void k_replay_importance(const int32_t *__restrict__ prio, int64_t batch, float beta,
                                                                          float *__restrict__ weights_out)
{
    GBL_FP_STRICT
    __shared__ uint32_t s_min[kImportanceThreads / 64];
    uint32_t mine = 0x7FFFFFFFu;
    for (int64_t j = threadIdx.x; j < batch; j += kImportanceThreads) {
        const int32_t p = prio[j];
        mine = p > 0 && (uint32_t)p < mine ? (uint32_t)p : mine;
    }
    mine = ~wave_max(~mine);
    if ((threadIdx.x & 63u) == 0u) s_min[threadIdx.x >> 6] = mine;
    __syncthreads();
    uint32_t wmin = s_min[0];
#pragma unroll
    for (int w = 1; w < kImportanceThreads / 64; ++w) wmin = s_min[w] < wmin ? s_min[w] : wmin;
    for (int64_t j = (int64_t)blockIdx.x * kImportanceThreads + threadIdx.x; j < batch; j += (int64_t)gridDim.x * kImportanceThreads)
        weights_out[j] = importance_weight(prio[j], (int32_t)wmin, beta);
}

// gbl_solve: the exact solver, one wavefront per board (a grid-stride loop over boards), three phases per board:
//   1. lane a < 54 plays root action a and, unless that decides it, every reply once (solve_root_action): depths 1 and 2 end here,
//      and so does every action with a reply that wins at once.  What is left of an action are its QUIET replies;
//   2. the (root action, quiet reply) pairs of the whole board are laid back to back -- an exclusive scan of the lanes' counts --
//      and dealt to the 64 lanes, each of which searches its pair's remaining depth - 2 plies serially in registers
//      (solve_reply) and folds the result into the action's order key with an LDS max;
//   3. lane a reads its action's key, the 54 result bytes go out one per lane, and a butterfly max decides.
// DEAL picks how phase 2 hands the pairs out: 0 = lane l takes pairs l, l + 64, ...; 1 = a lane takes the next pair off a counter
// in LDS whenever it is free.  Either way a lane's pairs come in ascending order, so the action of a pair is found by walking a
// cursor over the scan.
// The three phases live in solve_board, which gbl_collect_search_solve's kernel runs too.
//
// The solver's LDS of one board's wavefront: the quiet replies and the order key per root action, the scan, the deal's counter
struct SolveLds {
    uint64_t deep[kActions];
    uint32_t start[kActions + 1], key[kActions], next;
};

// Orders a wavefront's accesses to SolveLds between the phases.  BLOCK: __syncthreads(), k_solve's own; else wave_lds_fence() --
// a kernel with trajectory stores in flight must not wait for them here (see pool_fence).
template <bool BLOCK>
__device__ __forceinline__ void solve_fence()
{
    if (BLOCK)
        __syncthreads();
    else
        wave_lds_fence();
}

// One board's solve; every lane of the board's one wavefront calls it with the same root / mover / cand / depth.  Returns the
// decision's key (solve_action_of / solve_value_of read it) in every lane and leaves in c lane a's result byte (kSolveNone for a
// non-candidate).  At depth > 2 the caller passes solve_fence<BLOCK>() before the next call rewrites L.
template <int DEAL, bool BLOCK>
__device__ __forceinline__ uint32_t solve_board(SolveLds &L, const Planes &root, int mover, uint64_t cand, int depth, uint32_t lane, int &c)
{
    const bool mine = lane < (uint32_t)kActions && ((cand >> lane) & 1ull);
    SolveRoot A{kSolveNone, 0u, 0ull};
    if (mine) A = solve_root_action(root, mover, lane, depth);
    if (depth > 2) {  // (wave-uniform)
        uint32_t upto = (uint32_t)__popcll(A.deep);  // inclusive scan of the pairs per action
#pragma unroll
        for (uint32_t o = 1; o < 64u; o <<= 1) {
            const uint32_t below = (uint32_t)__shfl_up((int)upto, o);
            upto += lane >= o ? below : 0u;
        }
        const uint32_t total = (uint32_t)__shfl((int)upto, 63);
        if (lane < (uint32_t)kActions) {
            L.deep[lane] = A.deep;
            L.key[lane] = A.key;
            L.start[lane + 1] = upto;
        }
        if (lane == 0) {
            L.start[0] = 0u;
            L.next = 0u;
        }
        solve_fence<BLOCK>();
        uint32_t a = 0;
        for (uint32_t i = DEAL ? atomicAdd(&L.next, 1u) : lane; i < total; i = DEAL ? atomicAdd(&L.next, 1u) : i + 64u) {
            while (L.start[a + 1] <= i) ++a;  // (start[54] = total > i: a stays below 54)
            // key[a] is read plainly while other lanes atomicMax it: a stale value is one the action held earlier, which
            // cuts less and gives the same key (solve_reply) -- it costs work, never the result
            const uint32_t rb = kth_bit64(L.deep[a], i - L.start[a]);
            atomicMax(&L.key[a], solve_reply(root, mover, a, rb, depth, L.key[a]));
        }
        solve_fence<BLOCK>();
        if (A.deep) A.c = solve_parent(solve_of_key(L.key[lane]));
    }
    c = A.c;
    return wave_max(mine ? solve_action_key(A.c, lane) : 0u);
}

template <int DEAL>
__global__ __launch_bounds__(64) void k_solve(const int8_t *__restrict__ state, const int8_t *__restrict__ to_move,
                                              const int8_t *__restrict__ mask, int8_t *__restrict__ outcome_out,
                                              int8_t *__restrict__ value_out, int32_t *__restrict__ action_out, int64_t n, int depth)
{
    __shared__ SolveLds s_solve;
    const uint32_t lane = threadIdx.x;
    for (int64_t b = blockIdx.x; b < n; b += gridDim.x) {
        const Planes root = board_planes(state, b, lane);
        const int mover = to_move[b] != 0;
        int c;
        const uint32_t best = solve_board<DEAL, true>(s_solve, root, mover, board_candidates(root, mover, mask, b, lane), depth, lane, c);
        if (outcome_out && lane < (uint32_t)kActions) outcome_out[b * kActions + lane] = (int8_t)c;
        if (lane == 0) {
            if (value_out) value_out[b] = (int8_t)solve_value_of(best);
            if (action_out) action_out[b] = solve_action_of(best);
        }
        if (depth > 2) solve_fence<true>();  // (before the next board rewrites the LDS arrays)
    }
}

// The tablebase in a self-play launch (gbl_collect_search_tb, gbl_collect_gumbel_tb): the probe in front of every ply that is judged
// or played from the table.  The probe is k_tb_probe's on the live planes: lane a < 54 takes action a, its successor's three look-ups go to `aux` in global
// memory and one byte comes from anywhere in the table (a 64-bit offset); a butterfly gives V and a*.  A TABLEBASE mover's ply is done
// there -- the set O is a ballot, its visits row a count in O's lanes, the sampled draw search_decide's rule on that row (the running
// sum through lane a is count times the members of O up to a) -- and neither the solver nor the tree runs; on a board the table does
// not hold the masked-random sampler moves.  The lane's outcome byte and V stay for the second lambda, which stores the three judge
// arrays (the played action's byte comes from its lane by a shuffle).
struct TbPlay {
    const uint8_t *aux;
    const int8_t *table;
    TbShape S;
    int mode, count, judge;  // judge: a judge array is given, every ply is probed
    int8_t *outcome, *value, *played;
};

// The table's part of a self-play ply, for k_collect_tb and k_collect_gumbel_tb (every lane of the board's wavefront calls it): where
// the ply is judged or its mover plays from the table, the verdict -- k_tb_probe of the live planes, no mask -- into tb_c (this lane's
// outcome byte) and tb_v; a TABLEBASE mover on a board the table holds is decided here (S.d) and the call returns true: nothing else
// runs for the ply.
__device__ __forceinline__ bool wave_tb_ply(const TbPlay &tb, const SearchBoard &B, int who, uint64_t legal, int policy, int sample_plies,
                                            uint64_t seed, uint64_t g, uint32_t q, uint32_t lane, int &tb_c, int &tb_v, SearchPly &S)
{
    if (tb.judge || policy == kPolicyTablebase) {  // (wave-uniform)
        const TbAux A = tb_aux(tb.aux);
        uint64_t cand = legal & tb_piece_actions(tb.S);
        if (tb_board_index(A, tb.S, B.p, who) < 0) cand = 0;
        const bool mine = lane < (uint32_t)kActions && ((cand >> lane) & 1ull);
        if (mine) tb_c = (int)(int8_t)tb_probe_action(A, tb.S, tb.table, B.p, who, lane);  // (the outcome byte: see tb_target_keeps)
        const uint32_t best = wave_max(mine ? tb_action_key(tb_c, lane) : 0u);
        tb_v = uniform(tb_value_of(best));
        if (policy == kPolicyTablebase && best) {
            const bool keep = mine && tb_target_keeps(tb_c, tb_v, tb.mode);
            const uint64_t kept = (uint64_t)__ballot(keep);
            const uint32_t sum = (uint32_t)tb.count * (uint32_t)__popcll(kept);
            S.d = SearchDecision{uniform(tb_action_of(best)), kHowTable, tb_play_value(tb_v, (int)sum), keep ? (uint32_t)tb.count : 0u};
            if (B.tabs < sample_plies) {
                const uint32_t run = (uint32_t)tb.count * (uint32_t)__popcll(kept & ((2ull << lane) - 1ull));
                const uint32_t k = __umulhi(draw32(seed, g, q, kStreamVisit), sum);
                const uint64_t over = (uint64_t)__ballot(run > k);
                S.d.action = over ? (int)__builtin_ctzll(over) : -1;
                S.d.how = kHowTableSampled;
            }
            return true;
        }
    }
    return false;
}

// The three judge arrays' cell of a ply, for the same two kernels: the lane's outcome byte, V, and the byte of the action the ply played
// (from its lane by a shuffle).
__device__ __forceinline__ void wave_tb_store(const TbPlay &tb, int64_t at, int tb_c, int tb_v, int action, uint32_t lane)
{
    if (tb.outcome && lane < (uint32_t)kActions) __builtin_nontemporal_store((int8_t)tb_c, tb.outcome + at * kActions + lane);
    if (tb.value && lane == 0) tb.value[at] = (int8_t)tb_v;
    if (tb.played) {
        const int a = uniform(action);  // (the action the ply played: search_plies steps with the same)
        const int c = __shfl(tb_c, a < 0 ? 0 : a);
        if (lane == 0) tb.played[at] = (int8_t)(a < 0 ? kSolveNone : c);
    }
}

// ---- the evaluator self-play family: k_collect_eval, k_collect_tb and k_collect_gumbel_tb are compositions of the
// pieces below in the order host_selfplay_run's lambda has them -- probe (wave_tb_ply), guard, search, the ply's stores;
// k_collect_solve and k_collect_gumbel_solve keep their own text and argument lists: from the pieces they measured slower.
// SelfplayArgs: what a kernel takes after `done` (the nine arguments before it stay plain, in this order: they fill the 16 preloaded
// dwords).  The two sides' values are spelt out, not arrays: the mover picks wave-uniformly, field by field, all in SGPRs.
struct SelfplayArgs {
    int64_t ply_stride, tile_stride;
    SearchTraj T;
    int32_t *root_value;  // the root's q and the network's prior row of every searched ply,
    uint8_t *priors;
    int8_t *outcome, *proven;  // ... and the guard's outcome row and V
    EvalNet net0, net1;
    int policy0, policy1;
    uint32_t iterations0, iterations1;
    int solve_depth0, solve_depth1;
    uint32_t noise0, noise1, considered0, considered1, most, explore;
    int sample_plies, illegal_mode;
    int64_t *counters;
    int32_t *turn;
    GumbelArgs gum;  // (considered is not read: the two sides' own stand above)
    TbPlay tb;
};

// The family's LDS: (most + 1) nodes, then as many prior rows (dynamic); s_h, the ply's two row images, the solver's: what a kernel touches
struct PlyLds {
    TreeNode *nodes;
    uint8_t *pri;
    uint32_t *h, *obs, *mask;
    SolveLds *solve;
};

__device__ __forceinline__ PlyLds ply_lds(uint32_t most)
{
    extern __shared__ uint4 s_tree[];
    __shared__ uint32_t s_h[kEvalMaxHidden / 4];
    __shared__ uint32_t s_obs[32], s_mask[16];
    __shared__ SolveLds s_solve;
    TreeNode *const nodes = reinterpret_cast<TreeNode *>(s_tree);
    return PlyLds{nodes, reinterpret_cast<uint8_t *>(nodes + most + 1), s_h, s_obs, s_mask, &s_solve};
}

// The solver's guard of a ply (every lane calls it): on a guarded side (solve_depth_m > 0) solve_board on the live planes.  A proven
// root (V != 0) plays the solver's action -- S.d is filled -- and searches nothing; an unproven one narrows the search to C.
struct GuardPly {
    uint64_t cand;     // what the ply's search may play: C, or the legal mask of an unguarded ply
    int proven, my_c;  // V, and this lane's outcome byte (GBL_SOLVE_NONE on an unguarded ply)
};

__device__ __forceinline__ GuardPly wave_guard_ply(const SelfplayArgs &a, SolveLds &s_solve, const SearchBoard &B, int who, uint64_t legal,
                                                   uint32_t lane, SearchPly &S)
{
    GuardPly G{legal, 0, kSolveNone};
    const int depth = who ? a.solve_depth1 : a.solve_depth0;
    if (depth > 0 && legal) {  // (wave-uniform)
        const uint32_t best = solve_board<knob::kSolveDeal, false>(s_solve, B.p, who, legal, depth, lane, G.my_c);
        if (depth > 2) solve_fence<false>();  // (before the next ply's solve rewrites the LDS arrays)
        G.proven = uniform(solve_value_of(best));
        if (G.proven) {
            const uint32_t its = who ? a.iterations1 : a.iterations0;
            const int act = uniform(solve_action_of(best));
            S.d = SearchDecision{act, kHowProven, (G.proven > 0 ? 128 : -128) * (int)its, lane == (uint32_t)act ? its : 0u};
        } else {
            G.cand = (uint64_t)__ballot(G.my_c == 0);
        }
    }
    return G;
}

// The search-and-decide ply of an EVAL_TREE mover over cand (every lane calls it; S is filled).  A feature is compiled out where its
// flag is false; no kernel has both.  NOISE: the side's root noise.  GUMBEL: a side with considered_m > 0 searches by the Gumbel root
// rule with call = the ply index: the rule decides (never the visit-proportional draw), how = GBL_HOW_GUMBEL, the visits row = the target.
template <bool NOISE, bool GUMBEL>
__device__ __forceinline__ void wave_search_ply(const SelfplayArgs &a, const PlyLds &L, const SearchBoard &B, int who, uint64_t cand,
                                                uint64_t seed, uint64_t g, uint32_t q, uint32_t lane, SearchPly &S)
{
    uint32_t mixed;  // (the root's own row; the trajectory keeps the network's)
    WaveGumbel gb{GumbelArgs{who ? a.considered1 : a.considered0, a.gum.noise, a.gum.visit_offset, a.gum.scale}, seed, g, q, 0, 0, 0ull};
    const WaveEval at_root = tree_eval_iterations<NOISE, GUMBEL>(L.nodes, L.pri, L.h, eval_net_pick(a.net0, a.net1, who), B.p, who, cand,
                                                                 who ? a.iterations1 : a.iterations0, a.explore, lane, S.count,
                                                                 RootNoise{who ? a.noise1 : a.noise0, seed, g, q}, mixed, &gb);
    S.pi = at_root.pi;
    S.root_q = at_root.q;
    const bool rule = GUMBEL && gb.G.considered != 0u;  // (wave-uniform) a Gumbel side's ply
    S.d = search_decide(L.nodes, lane, !rule && B.tabs < a.sample_plies, seed, g, q);
    if constexpr (GUMBEL) {
        if (rule) {
            const GumbelOut out = wave_gumbel_out(gb, L.nodes, cand, at_root.q, lane);
            S.d.action = out.action;
            S.d.how = kHowGumbel;
            S.d.my_n = out.target;
        }
    }
    wave_lds_fence();  // (the root's children are read before the next search rewrites the tree)
}

// A ply's cell of the family's own trajectory arrays (wavefront 0): the root's q and the prior byte; the guard's outcome byte and V.
__device__ __forceinline__ void store_root_ply(const SelfplayArgs &a, int64_t at, const SearchPly &S, uint32_t lane)
{
    if (a.root_value && lane == 0) a.root_value[at] = S.root_q;
    if (a.priors && lane < (uint32_t)kActions) __builtin_nontemporal_store((uint8_t)S.pi, a.priors + at * kActions + lane);
}

__device__ __forceinline__ void store_guard_ply(const SelfplayArgs &a, int64_t at, int my_c, int proven, uint32_t lane)
{
    if (a.outcome && lane < (uint32_t)kActions) __builtin_nontemporal_store((int8_t)my_c, a.outcome + at * kActions + lane);
    if (a.proven && lane == 0) a.proven[at] = (int8_t)proven;
}

// gbl_collect_search_eval, and (GUMBEL) gbl_collect_search_gumbel with a Gumbel side: the search alone.
template <bool GUMBEL>
__global__ __launch_bounds__(64) void k_collect_eval(int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n, uint64_t seed,
                                                     uint64_t env_base, const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies,
                                                     int8_t *__restrict__ done, const SelfplayArgs a)
{
    const PlyLds L = ply_lds(a.most);
    const uint32_t lane = threadIdx.x;
    search_plies(
        state, to_move, done, a.turn, a.counters, n, seed, env_base, ply_dev, ply0, plies, a.ply_stride, a.tile_stride, a.T, a.illegal_mode,
        L.mask, L.obs,
        [&](const SearchBoard &B, int who, uint64_t legal, uint64_t g, uint32_t q, SearchPly &S) {
            if ((who ? a.policy1 : a.policy0) != kPolicyEvalTree) return false;
            wave_search_ply<false, GUMBEL>(a, L, B, who, legal, seed, g, q, lane, S);
            return true;
        },
        [&](int64_t at, const SearchPly &S) { store_root_ply(a, at, S, lane); });
}

// gbl_collect_search_solve: k_collect_eval with the exact solver in front of every search of a guarded side (solve_depth_m > 0).
// One wavefront per board (a grid-stride loop over boards), the ply loop inside (search_plies).  A guarded ply runs solve_board
// on the live planes.  A proven root (V != 0) plays the solver's action and searches nothing; an unproven root searches exactly as
// k_tree_eval does under the mask C = the actions of outcome 0 (tree_eval_iterations with cand = C, then search_decide).  The
// solver's LDS stands beside the tree's, and its fences are wave_lds_fence: the ply's trajectory stores stay in flight over the
// next decision.  The solver's registers are dead before the tree's come alive.  The outcome byte of every lane and V go out
// from the second lambda, beside the root's q and the prior byte.
// CAP (gbl_collect_search_cap): the ply that goes on to search first takes its budget and noise weight from cap_ply -- one generator
// word of the board's own stream, wave-uniform, so a budget that differs between plies and boards costs no divergence -- and a fast
// ply leaves a zero visits row and its own `how` codes.  CAP = false compiles all of it out: the kernels without it are the code they were.
template <bool NOISE, bool CAP>
__global__ __launch_bounds__(64) void k_collect_solve(int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n, uint64_t seed,
                                                      uint64_t env_base, const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies,
                                                      int8_t *__restrict__ done, int64_t ply_stride, int64_t tile_stride, SearchTraj T,
                                                      int32_t *__restrict__ root_value_traj, uint8_t *__restrict__ priors_traj,
                                                      int8_t *__restrict__ outcome_traj, int8_t *__restrict__ proven_traj,
                                                      const EvalNet net0, const EvalNet net1, int policy0, int policy1, uint32_t iterations0,
                                                      uint32_t iterations1, int solve_depth0, int solve_depth1, uint32_t most, uint32_t explore,
                                                      int sample_plies, int illegal_mode, int64_t *__restrict__ counters,
                                                      int32_t *__restrict__ turn, uint32_t noise0, uint32_t noise1, uint32_t fast0,
                                                      uint32_t fast1, uint32_t share0, uint32_t share1)
{
    extern __shared__ uint4 s_tree[];
    TreeNode *const nodes = reinterpret_cast<TreeNode *>(s_tree);
    uint8_t *const pri = reinterpret_cast<uint8_t *>(nodes + most + 1);
    __shared__ uint32_t s_h[kEvalMaxHidden / 4];
    __shared__ uint32_t s_obs[32], s_mask[16];  // the ply's observation row (117 bytes) and mask row (54)
    __shared__ SolveLds s_solve;
    const uint32_t lane = threadIdx.x;
    int my_c = kSolveNone, proven = 0;  // the ply's outcome byte of this lane and V, from the first lambda to the second
    search_plies(
        state, to_move, done, turn, counters, n, seed, env_base, ply_dev, ply0, plies, ply_stride, tile_stride, T, illegal_mode, s_mask, s_obs,
        [&](const SearchBoard &B, int who, uint64_t legal, uint64_t g, uint32_t q, SearchPly &S) {
            my_c = kSolveNone;
            proven = 0;
            if ((who ? policy1 : policy0) != kPolicyEvalTree) return false;
            const uint32_t its = who ? iterations1 : iterations0;
            const int depth = who ? solve_depth1 : solve_depth0;
            uint64_t cand = legal;
            if (depth > 0 && legal) {  // (wave-uniform)
                const uint32_t best = solve_board<knob::kSolveDeal, false>(s_solve, B.p, who, legal, depth, lane, my_c);
                if (depth > 2) solve_fence<false>();  // (before the next ply's solve rewrites the LDS arrays)
                proven = uniform(solve_value_of(best));
                if (proven) {
                    const int a = uniform(solve_action_of(best));
                    S.d = SearchDecision{a, kHowProven, (proven > 0 ? 128 : -128) * (int)its, lane == (uint32_t)a ? its : 0u};
                    return true;
                }
                cand = (uint64_t)__ballot(my_c == 0);
            }
            CapPly cp{false, its, who ? noise1 : noise0};
            if (CAP) {  // the ply's budget and weight, after the guard: one generator word, the same in every lane
                cp = cap_ply(seed, g, q, who ? share1 : share0, its, who ? fast1 : fast0, cp.noise);
                cp = CapPly{uniform((int)cp.fast) != 0, (uint32_t)uniform((int)cp.its), (uint32_t)uniform((int)cp.noise)};
            }
            uint32_t mixed;  // (the root's own row; the trajectory keeps the network's)
            const WaveEval at_root = tree_eval_iterations<NOISE>(nodes, pri, s_h, eval_net_pick(net0, net1, who), B.p, who, cand, cp.its,
                                                                 explore, lane, S.count, RootNoise{cp.noise, seed, g, q}, mixed);
            S.pi = at_root.pi;
            S.root_q = at_root.q;
            S.d = search_decide(nodes, lane, B.tabs < sample_plies, seed, g, q);
            if (CAP && cp.fast) {  // (kHowSearch -> kHowFast, kHowSearchSampled -> kHowFastSampled; no policy target)
                S.d.how += kHowFast - kHowSearch;
                S.d.my_n = 0u;
            }
            wave_lds_fence();  // (the root's children are read before the next search rewrites the tree)
            return true;
        },
        [&](int64_t at, const SearchPly &S) {
            if (root_value_traj && lane == 0) root_value_traj[at] = S.root_q;
            if (priors_traj && lane < (uint32_t)kActions) __builtin_nontemporal_store((uint8_t)S.pi, priors_traj + at * kActions + lane);
            if (outcome_traj && lane < (uint32_t)kActions) __builtin_nontemporal_store((int8_t)my_c, outcome_traj + at * kActions + lane);
            if (proven_traj && lane == 0) proven_traj[at] = (int8_t)proven;
        });
}

// gbl_collect_gumbel_solve: k_collect_solve<false, false> with the Gumbel root rule on the unproven ply -- the kernel of a call that has
// both a guarded side and a Gumbel side (selfplay_launch runs k_collect_eval<true> or k_collect_solve<false, false> for every other
// call of the entry point, so neither of them carries the other's code).  A guarded ply is k_collect_solve's: solve_board on the live
// planes, a proven root plays the solver's action and neither searches nor draws.  The ply that goes on searches over cand = C (the
// actions of outcome 0; the legal mask of an unguarded side) exactly as k_collect_eval<true> does over the legal mask:
// tree_eval_iterations<false, true>, and for a side with considered_m > 0 wave_gumbel_finish on the root's read-out -- ply q's search IS
// gbl_tree_search_gumbel(mask = C, call = q).  A side with considered_m == 0 decides by search_decide, sample_plies honoured.  The
// solver's registers are dead before the tree's come alive; its LDS stands beside the tree's, fenced by wave_lds_fence.  gum.G's
// considered is not read: the two sides' own travel beside it.
__global__ __launch_bounds__(64) void k_collect_gumbel_solve(int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n, uint64_t seed,
                                                             uint64_t env_base, const uint32_t *__restrict__ ply_dev, uint32_t ply0,
                                                             uint32_t plies, int8_t *__restrict__ done, int64_t ply_stride,
                                                             int64_t tile_stride, SearchTraj T, int32_t *__restrict__ root_value_traj,
                                                             uint8_t *__restrict__ priors_traj, int8_t *__restrict__ outcome_traj,
                                                             int8_t *__restrict__ proven_traj, const EvalNet net0, const EvalNet net1,
                                                             int policy0, int policy1, uint32_t iterations0, uint32_t iterations1,
                                                             int solve_depth0, int solve_depth1, uint32_t most, uint32_t explore,
                                                             int sample_plies, int illegal_mode, int64_t *__restrict__ counters,
                                                             int32_t *__restrict__ turn, const GumbelArgs gum, uint32_t considered0,
                                                             uint32_t considered1)
{
    extern __shared__ uint4 s_tree[];
    TreeNode *const nodes = reinterpret_cast<TreeNode *>(s_tree);
    uint8_t *const pri = reinterpret_cast<uint8_t *>(nodes + most + 1);
    __shared__ uint32_t s_h[kEvalMaxHidden / 4];
    __shared__ uint32_t s_obs[32], s_mask[16];  // the ply's observation row (117 bytes) and mask row (54)
    __shared__ SolveLds s_solve;
    const uint32_t lane = threadIdx.x;
    int my_c = kSolveNone, proven = 0;  // the ply's outcome byte of this lane and V, from the first lambda to the second
    search_plies(
        state, to_move, done, turn, counters, n, seed, env_base, ply_dev, ply0, plies, ply_stride, tile_stride, T, illegal_mode, s_mask, s_obs,
        [&](const SearchBoard &B, int who, uint64_t legal, uint64_t g, uint32_t q, SearchPly &S) {
            my_c = kSolveNone;
            proven = 0;
            if ((who ? policy1 : policy0) != kPolicyEvalTree) return false;
            const uint32_t its = who ? iterations1 : iterations0;
            const int depth = who ? solve_depth1 : solve_depth0;
            uint64_t cand = legal;
            if (depth > 0 && legal) {  // (wave-uniform)
                const uint32_t best = solve_board<knob::kSolveDeal, false>(s_solve, B.p, who, legal, depth, lane, my_c);
                if (depth > 2) solve_fence<false>();  // (before the next ply's solve rewrites the LDS arrays)
                proven = uniform(solve_value_of(best));
                if (proven) {
                    const int a = uniform(solve_action_of(best));
                    S.d = SearchDecision{a, kHowProven, (proven > 0 ? 128 : -128) * (int)its, lane == (uint32_t)a ? its : 0u};
                    return true;
                }
                cand = (uint64_t)__ballot(my_c == 0);
            }
            uint32_t mixed;  // (no noise here: the network's byte)
            WaveGumbel gb{GumbelArgs{who ? considered1 : considered0, gum.noise, gum.visit_offset, gum.scale}, seed, g, q, 0, 0, 0ull};
            const WaveEval at_root = tree_eval_iterations<false, true>(nodes, pri, s_h, eval_net_pick(net0, net1, who), B.p, who, cand, its,
                                                                       explore, lane, S.count, RootNoise{}, mixed, &gb);
            S.pi = at_root.pi;
            S.root_q = at_root.q;
            const bool rule = gb.G.considered != 0u;  // (wave-uniform) a Gumbel side's ply
            S.d = search_decide(nodes, lane, !rule && B.tabs < sample_plies, seed, g, q);
            if (rule) {
                GumbelOut out{-1, 0u};
                if (gb.A) out = wave_gumbel_finish(gb, tree_lane_child(nodes, nodes[0].child, lane), cand, at_root.q, lane);
                S.d.action = out.action;
                S.d.how = kHowGumbel;
                S.d.my_n = out.target;
            }
            wave_lds_fence();  // (the root's children are read before the next search rewrites the tree)
            return true;
        },
        [&](int64_t at, const SearchPly &S) {
            if (root_value_traj && lane == 0) root_value_traj[at] = S.root_q;
            if (priors_traj && lane < (uint32_t)kActions) __builtin_nontemporal_store((uint8_t)S.pi, priors_traj + at * kActions + lane);
            if (outcome_traj && lane < (uint32_t)kActions) __builtin_nontemporal_store((int8_t)my_c, outcome_traj + at * kActions + lane);
            if (proven_traj && lane == 0) proven_traj[at] = (int8_t)proven;
        });
}

// gbl_collect_search_tb: the table's probe in front of every ply that is judged or played from it, the judge's arrays behind the guard's.
// SEARCH = false is the launch without an EVAL_TREE side: the solver and the tree are compiled out, and with them their registers and
// LDS -- such a ply is a chain of dependent look-ups that only more resident wavefronts hide.
template <bool NOISE, bool SEARCH>
__global__ __launch_bounds__(64) void k_collect_tb(int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n, uint64_t seed,
                                                   uint64_t env_base, const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies,
                                                   int8_t *__restrict__ done, const SelfplayArgs a)
{
    const PlyLds L = ply_lds(a.most);
    const uint32_t lane = threadIdx.x;
    int my_c = kSolveNone, proven = 0;  // the ply's outcome byte of this lane and V, from the first lambda to the second
    int tb_c = kSolveNone, tb_v = 0;  // the table's outcome byte of this lane and V, from the first lambda to the second
    search_plies(
        state, to_move, done, a.turn, a.counters, n, seed, env_base, ply_dev, ply0, plies, a.ply_stride, a.tile_stride, a.T, a.illegal_mode,
        L.mask, L.obs,
        [&](const SearchBoard &B, int who, uint64_t legal, uint64_t g, uint32_t q, SearchPly &S) {
            my_c = kSolveNone;
            proven = 0;
            tb_c = kSolveNone;
            tb_v = 0;
            const int policy = who ? a.policy1 : a.policy0;
            if (wave_tb_ply(a.tb, B, who, legal, policy, a.sample_plies, seed, g, q, lane, tb_c, tb_v, S)) return true;
            if (!SEARCH || policy != kPolicyEvalTree) return false;
            if constexpr (SEARCH) {
                const GuardPly G = wave_guard_ply(a, *L.solve, B, who, legal, lane, S);
                my_c = G.my_c;
                proven = G.proven;
                if (!proven) wave_search_ply<NOISE, false>(a, L, B, who, G.cand, seed, g, q, lane, S);
            }
            return true;
        },
        [&](int64_t at, const SearchPly &S) {
            store_root_ply(a, at, S, lane);
            store_guard_ply(a, at, my_c, proven, lane);
            wave_tb_store(a.tb, at, tb_c, tb_v, S.d.action, lane);
        });
}

// gbl_collect_gumbel_tb: the kernel of a call that has a Gumbel side and reads the table (every other call of the entry point runs
// k_collect_eval<true> or k_collect_tb).  Only the lane's outcome byte and V live across the search; no solver and no noise here.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_collect_gumbel_tb(
    int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n, uint64_t seed, uint64_t env_base,
    const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies, int8_t *__restrict__ done, const SelfplayArgs a)
{
    const PlyLds L = ply_lds(a.most);
    const uint32_t lane = threadIdx.x;
    int tb_c = kSolveNone, tb_v = 0;  // the table's outcome byte of this lane and V, from the first lambda to the second
    search_plies(
        state, to_move, done, a.turn, a.counters, n, seed, env_base, ply_dev, ply0, plies, a.ply_stride, a.tile_stride, a.T, a.illegal_mode,
        L.mask, L.obs,
        [&](const SearchBoard &B, int who, uint64_t legal, uint64_t g, uint32_t q, SearchPly &S) {
            tb_c = kSolveNone;
            tb_v = 0;
            const int policy = who ? a.policy1 : a.policy0;
            if (wave_tb_ply(a.tb, B, who, legal, policy, a.sample_plies, seed, g, q, lane, tb_c, tb_v, S)) return true;
            if (policy != kPolicyEvalTree) return false;
            wave_search_ply<false, true>(a, L, B, who, legal, seed, g, q, lane, S);
            return true;
        },
        [&](int64_t at, const SearchPly &S) {
            store_root_ply(a, at, S, lane);
            wave_tb_store(a.tb, at, tb_c, tb_v, S.d.action, lane);
        });
}

// gbl_greedy: one decision per board.  Each lane owns a board (depth-1 walk, order-dependent replay,
// fallback test), but the depth-2 evaluations -- one moved + legal54 + outcomes54 per (board,
// candidate) pair, ~95 % of the work -- are pooled over the tile: the boards' candidate lists are
// laid back to back in LDS and lane l evaluates pairs l, l+64, ... whoever owns them, so a
// wavefront runs ceil(total / 64) evaluations instead of as many as its busiest board has candidates
// (~50 against a mean of ~33 on the masked-random mix).
// W wavefronts per workgroup share one tile: wavefront 0 owns the boards (loads, depth-1 walk, replay,
// outputs), all W evaluate pairs, so a tile's serial chain shrinks and every SIMD holds wavefronts in
// different phases.  W = 1 needs no barrier (depth 1 has no pairs and uses it).
// Orders the workgroup's LDS accesses (the only thing the wavefronts of a tile share).  Not __syncthreads(): that also
// waits for the caller's outstanding global stores (vmcnt), which in gbl_collect_policy would put the drain of a ply's
// trajectory stores on the path of the next decision.
template <int W>
__device__ __forceinline__ void pool_fence()
{
    if (W > 1)
        pair_barrier();
    else
        wave_lds_fence();
}

// ---- the greedy decision of a BLOCK of NT tiles (64 NT boards) by a workgroup of W wavefronts -----------------------------
// Wavefronts 0 .. NT-1 each OWN a tile (lane = board: loads, depth-1 walk, replay, outputs); wavefronts NT .. 2 NT - 1 look at
// the same tiles from the opponent's side while the owners walk depth 1; ALL W wavefronts lay out and evaluate the block's
// depth-2 work, whoever owns it (wavefronts beyond 2 NT do nothing else).  Shapes: <1, 16> / <1, 8> a lone tile spread over
// many wavefronts (small batches: the shortest serial chain), <1, 4> the same over four (large batches: the smallest
// workgroups), <2, 8> / <4, 8> / <4, 16>: blocks of tiles -- as many owners as helpers, so that fewer of a CU's wavefronts
// idle through the owners' phases (the tiles of a CU run in step) -- for batches of one generation of tiles; <1, 1>: depth 1
// only, no shared phase, no barrier.  greedy_shape() / policy_shape() hold the measurements behind the choice.
template <int NT, int W>
struct GreedyLds {
    static_assert(W == 1 || W >= 2 * NT, "a helper wavefront per owner");
    static constexpr int kBoards = kTile * NT;
    static_assert(kBoards <= 256, "(board << 8) | candidate fits 16 bits");
    // An owner's output image of gbl_collect_policy (scratch(), below) is staged in the pair list, which is padded so that NT images fit it
    static constexpr int kImageBytes = 4 * image_words<kObs>();
    static constexpr int kPairSlots = kBoards * kActions;
    static constexpr int kPairPad = NT * kImageBytes > 2 * kPairSlots ? (NT * kImageBytes - 2 * kPairSlots) / 2 : 0;
    alignas(16) uint16_t pair[kPairSlots + kPairPad]; // (board << 8) | candidate of every depth-2 evaluation of the block: those that
                                                      // take the fast form from the front, the ORDERED form (greedy_nonplain) from the back
                                                      // (the back = slot kPairSlots - 1; the padding behind it is scratch only)
    unsigned long long undef[kBoards][kRootItems];    // per board and member j of the root's replies: greedy_undefused
    uint16_t item[kBoards * kRootItems];              // (board << 8) | j of every member of a root's replies that is dealt out
    uint32_t board[kBoards][4];            // planes nz, neg, odd; bit 0: the agent to move, bit 1: the board wants depth 2
    uint64_t legal[kBoards];               // its legal moves on the root position
    unsigned long long work[kBoards];      // w0 = todo & ~dup: the candidates of a board that want a reply summary (see plan_of)
    unsigned long long replies[kBoards];   // the opponent's winning moves on the root (greedy_root); after the plan: those dealt out
    uint32_t risky[kBoards];               // 9 bits: squares where a placement from hand has to be evaluated (greedy_root)
    int npairs, nitems;                    // npairs: fast pairs in the low, ordered pairs in the high 16 bits
    uint16_t reply[kBoards][kActions];     // greedy_reply() of (board, candidate), where bit 0 is set
    unsigned long long threat[kBoards];    // candidates whose summary has bit 0 / bit 15 / bit 7 / bit 8,
    unsigned long long allwin[kBoards];    // and those whose first winning reply is a legal move of ours
    unsigned long long second[kBoards];    // (the sets greedy_replay_closed works on)
    unsigned long long block[kBoards];
    unsigned long long flegal[kBoards];
    unsigned long long nonplain[kBoards];  // greedy_nonplain of the board
    int job;                               // the next chunk of 64 pairs / items to hand out
    // The pair list is dead between two decisions (written after the third barrier of greedy_tile, read before its last one): a
    // kernel that decides in a loop stages its owners' output rows through it in between, owner w through bytes
    // [w, w + 1) * kImageBytes of it.  ONLY the pair list: the table `undef` is still read by every owner after the last
    // barrier (greedy_hand_merge), so an image laid over it -- round 3's layout: the list and the table as one region cut
    // in NT equal slices -- let a fast owner's next image overwrite a slower owner's rows (no barrier orders the two).
    static_assert(kImageBytes % 16 == 0 && NT * kImageBytes <= (int)sizeof(pair), "NT output images fit the (padded) pair list");
    __device__ __forceinline__ uint32_t *scratch(int owner_wave)
    {
        return reinterpret_cast<uint32_t *>(pair) + owner_wave * (kImageBytes / 4);
    }
};

// Inclusive prefix sum over the 64 lanes of a wavefront in six DPP adds (Hillis-Steele inside the rows of 16, then the rows'
// totals: lane 15 of a row into the next one, lane 31 into rows 2 and 3); scripts/microbench/dpp_scan.hip checks it on the GPU.
__device__ __forceinline__ uint32_t wave_incl_scan_add(uint32_t x)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return x;
}

// Compacts the (board, step) entries of a wavefront's lanes -- lane = board, `bits` = the steps (candidates / ranks) it has
// -- into a list shared by the whole block.  The lanes' counts are prefix-summed with six DPP adds (round 3: bit-sliced, one
// ballot + two mbcnt per bit of the largest possible count); the wavefront reserves its stretch of the list with ONE atomic,
// and a lane writes its few entries in a loop (as long as the busiest lane's count: 4-6 of 14 steps).  Round 3's first form --
// one ballot + mbcnt + store per STEP, in two passes around the atomic -- cost a wavefront 2 400 cycles (per-wavefront stamps),
// five barriers' worth.  (Every lane of the wavefront must be active: both callers are wave-uniform branches.)
template <int STEPS>
__device__ __forceinline__ void list_append(uint16_t *list, int *fill, uint32_t tag, int lane, uint32_t bits)
{
    static_assert(STEPS <= 31, "the steps of a lane fit a 32-bit set");
    const uint32_t cnt = (uint32_t)__popc(bits);
    const uint32_t inc = wave_incl_scan_add(cnt);
    uint32_t base = 0;
    if (lane == kTile - 1 && inc) base = (uint32_t)atomicAdd(fill, (int)inc);
    uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)base, kTile - 1) + inc - cnt;
    for (uint32_t rest = bits; rest; rest &= rest - 1u) list[at++] = (uint16_t)(tag + (uint32_t)__builtin_ctz(rest));
}

// list_append for two lists at once -- entries of `bits` go to `list` upwards, those of `bitsx` (few lanes have any) from
// `listx` DOWNWARDS (the two share one array) -- whose fill counts share one word (low / high 16 bits): one scan of the packed
// counts, one atomic per wavefront.
template <int STEPS>
__device__ __forceinline__ void list_append2(uint16_t *list, uint16_t *listx, int *fill, uint32_t tag, int lane, uint64_t bits, uint64_t bitsx)
{
    static_assert(STEPS <= 63, "the steps of a lane fit a 64-bit set");
    const uint32_t cnt = STEPS < 32 ? (uint32_t)__popc((uint32_t)bits) : (uint32_t)__popcll(bits);
    const uint32_t cntx = STEPS < 32 ? (uint32_t)__popc((uint32_t)bitsx) : (uint32_t)__popcll(bitsx);
    const uint32_t own = cnt | (cntx << 16);          // (a wavefront's totals are < 2^16 each: no carry between the halves)
    const uint32_t inc = wave_incl_scan_add(own);
    uint32_t base = 0;
    if (lane == kTile - 1 && inc) base = (uint32_t)atomicAdd(fill, (int)inc);
    const uint32_t start = (uint32_t)__builtin_amdgcn_readlane((int)base, kTile - 1) + inc - own;
    uint32_t at = start & 0xFFFFu, atx = start >> 16;
    if (STEPS < 32) {
        for (uint32_t rest = (uint32_t)bits; rest; rest &= rest - 1u) list[at++] = (uint16_t)(tag + (uint32_t)__builtin_ctz(rest));
        for (uint32_t rest = (uint32_t)bitsx; rest; rest &= rest - 1u) listx[-(int)(atx++)] = (uint16_t)(tag + (uint32_t)__builtin_ctz(rest));
    } else {
        for (uint64_t rest = bits; rest; rest &= rest - 1ull) list[at++] = (uint16_t)(tag + (uint32_t)__builtin_ctzll(rest));
        for (uint64_t rest = bitsx; rest; rest &= rest - 1ull) listx[-(int)(atx++)] = (uint16_t)(tag + (uint32_t)__builtin_ctzll(rest));
    }
}

// One decision per board of the block, by ALL 64 W threads of the workgroup (every thread calls, the barriers are inside).
// The owners (wave < NT, lane = board of their tile) pass their board, the agent to move, the legal mask handed to the
// policy (0: nothing to decide on this board -- an invalid lane, or in gbl_collect_policy a board whose mover plays at
// random), the board's depth (1, 2; 3 decides like 2) and the agent's last three actions; the other threads' arguments are
// ignored and they get an empty result.  deep: some board of SOME block of the launch may want depth 2 (workgroup-uniform:
// it decides whether the shared phases and their barriers exist at all; W == 1 has none).
//
// Depth 2 in five steps between barriers:  (A) the owners publish their boards;  (B) they walk depth 1 (greedy_head) while
// their helpers find the opponent's winning moves on the root and the risky squares (greedy_root) and a third wavefront per
// tile the moves of ours after which a reply could expose a line of ours (greedy_nonplain);  (C) the owners split their
// candidates (greedy_root_plan): placements from hand on non-risky squares are settled from the root's replies R, everything
// else is evaluated -- in the FAST form (threat squares) unless greedy_nonplain says otherwise;  (D) all wavefronts lay out the
// work -- the (board, candidate) pairs, fast ones from the front of the list and ordered ones from its back, and the (board,
// member of R) items;  (E) the work goes out in chunks of 64 through a counter -- ordered pairs, fast pairs (one moved +
// legal54 + wins54_plain / outcomes54 each: every reply's result at once), items (greedy_undefused) -- to whichever wavefront
// is free, leaving 16-bit summaries, candidate-set bits and table rows in LDS; then the owners replay the reference's depth-2
// loop in closed form over the sets (greedy_replay_closed).
// Safe to call in a loop: what the owners read last (replay) and write first (heads) is their own wavefront's business,
// and everybody else's reads of an iteration lie before its last barrier.
// (kSkip: 0 in the product.  The FLOOR builds of scripts/greedy_floor.sh -- experiment builds, gobblet_ab.h -- leave phases of the
// decision out, with WRONG results, so that what a block cannot go below is measured, not argued.)
template <int NT, int W>
__device__ __forceinline__ GreedyResult greedy_tile(GreedyLds<NT, W> &S, const Planes &p, int me, uint64_t mask, int depth,
                                                    bool deep, uint32_t prev3, TileStamps &ts)
{
    constexpr int kSkip = knob::kGreedySkip;
    const int lane = (int)(threadIdx.x & 63u), wave = wave_index();
    const bool owner = wave < NT;
    const int bi = (owner ? wave : wave - NT) * kTile + lane;  // the board this thread owns, or helps with (wave < 2 NT)
    GreedyHead h{0ull, 0ull, 0ull, 0ull, 0, -1};
    GreedyRootPlan plan{0ull, 0ull, 0ull};
    const bool two = owner && depth > 1 && mask != 0;  // this board takes part in the depth-2 round
    if constexpr (W == 1) {
        (void)S; (void)deep; (void)ts; (void)bi; (void)two;
        h = greedy_head(p, me, mask, 1);  // (one wavefront: depth 1 only -- the hosts never launch it for more)
        return greedy_finish(h, prev3);
    } else {
    if (owner && deep) {
        S.board[bi][0] = p.nz;
        S.board[bi][1] = p.neg;
        S.board[bi][2] = p.odd;
        S.board[bi][3] = (uint32_t)me | (two ? 2u : 0u);
        if (threadIdx.x == 0) {
            S.npairs = 0;
            S.nitems = 0;
            S.job = 0;
        }
    }
    if (deep) {
        GBL_WAVE_STAMP(8);
        pool_fence<W>();
        GBL_WAVE_STAMP(9);
        // (B) the helpers look at the root from the OPPONENT's side (as expensive as the depth-1 walk itself)
        if (!(kSkip & 8) && wave >= NT && wave < 2 * NT && (S.board[bi][3] & 2u)) {
            const Planes q{S.board[bi][0], S.board[bi][1], S.board[bi][2]};
            const GreedyRoot g = greedy_root(q, (int)(S.board[bi][3] & 1u));
            S.replies[bi] = g.replies;
            S.risky[bi] = g.risky;
        }
        // ... and a wavefront that would idle (blocks without one: the helpers, on top) finds the moves of ours after which
        // a reply could expose a line of ours: those pairs take the ordered form of the evaluation, all others the fast one
        constexpr int kPlainWave0 = W >= 3 * NT ? 2 * NT : NT;
        if (!(kSkip & 8) && wave >= kPlainWave0 && wave < kPlainWave0 + NT) {
            const int bn = (wave - kPlainWave0) * kTile + lane;
            if (S.board[bn][3] & 2u)
                S.nonplain[bn] = greedy_nonplain(Planes{S.board[bn][0], S.board[bn][1], S.board[bn][2]}, (int)(S.board[bn][3] & 1u));
        }
    }
    if (owner) {
        if (!(kSkip & 8)) h = greedy_head(p, me, mask, depth);  // empty mask: nothing to do
        if (deep) {
            S.legal[bi] = h.legal_me;
            S.threat[bi] = 0ull;
            S.allwin[bi] = 0ull;
            S.second[bi] = 0ull;
            S.block[bi] = 0ull;
            S.flegal[bi] = 0ull;
        }
    }
    // (C) The split of a board's candidates -- twin placements are not evaluated a second time; placements from hand on non-risky
    // squares not at all, they are settled from the root's replies; the rest in the fast or the ordered form -- needs the owner's
    // depth-1 result (w0 = todo & ~dup) and the helpers' findings.  Round 4 had the owners compute it alone between two barriers
    // (1.7 k cycles of a 21.8 k block with one wavefront per SIMD at work); round 5: the owners publish w0 with their other results
    // before barrier B, and whoever needs the split of a board afterwards -- the listing wavefronts for the boards they list, the
    // owners for their own -- derives it from LDS (~40 instructions, in the throughput-bound list phase): one barrier less.
    // Measured (scripts/ab_greedy.py, in-process, us per launch old -> new): <1,16> at 4 096 boards 8.96 -> 8.25, <2,8> at 32 768:
    // 10.65 -> 10.02 (gbl_collect_policy 10.67 -> 10.10 per ply); <4,16> at 65 536: 12.05 -> 12.25 and <1,4> at 2^20: 143.3 -> 144.8
    // -- blocks that fill their SIMDs pay for the sixteen (four) copies of the split more than the barrier cost them: they keep
    // round 4's flow (kListerPlan false).
    constexpr bool kListerPlan = (NT == 1 && W >= 8) || (NT == 2);
    if (kListerPlan && owner && deep) S.work[bi] = two ? (h.todo & ~h.dup) : 0ull;
    auto plan_of = [&](int bn) {
        const unsigned long long w0 = S.work[bn];
        const Planes q{S.board[bn][0], S.board[bn][1], S.board[bn][2]};
        const GreedyRoot gr{S.replies[bn], S.risky[bn]};
        const bool rule = __popcll(gr.replies) <= kRootItems;
        const uint64_t resolved = rule ? (w0 & greedy_from_hand(q, (int)(S.board[bn][3] & 1u)) & ~spread9(gr.risky)) : 0ull;
        return GreedyRootPlan{w0 & ~resolved, resolved, resolved ? gr.replies : 0ull};
    };
    GBL_TILE_STAMP(ts, 0);
    if (deep) {
        GBL_WAVE_STAMP(10);
        pool_fence<W>();  // the helpers' findings and the owners' depth-1 results are in
        if constexpr (kListerPlan) {
            if (two) plan = plan_of(bi);
        } else {
            if (owner) {  // the owners alone, between two barriers: S.work = the split's `eval` set itself
                if (two) plan = greedy_root_plan(h, p, me, GreedyRoot{S.replies[bi], S.risky[bi]});
                S.work[bi] = plan.eval;
                S.replies[bi] = plan.items;
            }
            GBL_WAVE_STAMP(0);
            pool_fence<W>();
        }
        GBL_WAVE_STAMP(1);
        // (D) the work lists: W / NT wavefronts share a tile's 54 candidate steps, and the owners take their tile's 6 rank
        // steps on top
        // (fewer listers with longer per-lane loops lose: two per tile +2 %, one per tile +12 % at 65 536 boards)
        constexpr int kWavesPerTile = W / NT, kSteps = (kActions + kWavesPerTile - 1) / kWavesPerTile;
        if (const int lw = wave - (W - NT * kWavesPerTile); lw >= 0 && !(kSkip & 4)) {  // (the last wavefronts: the owners come out of the plan last)
            const int g = lw / kWavesPerTile, c0 = (lw % kWavesPerTile) * kSteps;  // (a wavefront's steps stay inside one tile)
            if (c0 < kActions) {
                const int steps = kActions - c0 < kSteps ? kActions - c0 : kSteps;
                const int bn = g * kTile + lane;
                const uint64_t ev = kListerPlan ? plan_of(bn).eval : (uint64_t)S.work[bn];
                const uint64_t slow = ev ? S.nonplain[bn] : 0ull;  // (the nonplain set exists for boards that take part)
                const uint64_t wk = ((ev & ~slow) >> c0) & ((1ull << steps) - 1ull);
                const uint64_t wx = ((ev & slow) >> c0) & ((1ull << steps) - 1ull);
                list_append2<kSteps>(S.pair, S.pair + (GreedyLds<NT, W>::kBoards * kActions - 1), &S.npairs,
                                     ((uint32_t)bn << 8) + (uint32_t)c0, lane, wk, wx);
            }
        }
        GBL_WAVE_STAMP(6);
        // (blocks of tiles: by the owners -- the oldest wavefronts on their SIMDs win the issue arbitration and are through
        // first; a lone tile: by its helper, the owner's own path being the longest there)
        constexpr int kItemWave0 = NT * kWavesPerTile < W ? 0 : NT == 1 ? 1 : 0;  // (wavefronts that list no pairs, if any)
        if (!(kSkip & 4) && wave >= kItemWave0 && wave < kItemWave0 + NT) {
            const int g = wave - kItemWave0, bn = g * kTile + lane;
            // (the owners list their own boards; a lone tile's helper reads, or derives, its board's)
            const uint32_t nr = (uint32_t)__popcll(!kListerPlan ? (uint64_t)S.replies[bn] : (kItemWave0 == 0 ? plan : plan_of(bn)).items);
            list_append<kRootItems>(S.item, &S.nitems, (uint32_t)bn << 8, lane, (1u << nr) - 1u);
        }
        GBL_WAVE_STAMP(7);
        pool_fence<W>();
        GBL_WAVE_STAMP(2);
        // (E) the work in chunks of 64, handed out through a counter -- the ordered pairs first (an ordered evaluation is
        // twice a fast one), then the fast pairs, then the items: whoever is through takes the next chunk, so the oldest
        // wavefronts of a SIMD, which win the issue arbitration, simply take more
        int nfast = S.npairs & 0xFFFF, nslow = (int)((uint32_t)S.npairs >> 16);
        const int nitems = S.nitems;
        if constexpr (knob::kGreedyPairCap > 0) {  // (floor builds only: pairs beyond the cap are dropped -- WRONG results, timing only)
            nslow = nslow < knob::kGreedyPairCap ? nslow : knob::kGreedyPairCap;
            nfast = nfast < knob::kGreedyPairCap - nslow ? nfast : knob::kGreedyPairCap - nslow;
        }
        const int jslow = (nslow + kTile - 1) / kTile, jfast = (nfast + kTile - 1) / kTile, jitem = (nitems + kTile - 1) / kTile;
        auto record = [&](uint32_t o, uint32_t a, uint32_t sum) {
            if (sum & 1u) {
                S.reply[o][a] = (uint16_t)sum;
                atomicOr(&S.threat[o], 1ull << a);
                if (sum & (1u << 7)) atomicOr(&S.second[o], 1ull << a);
                if (sum & (1u << 8)) atomicOr(&S.block[o], 1ull << a);
                if ((S.legal[o] >> ((sum >> 1) & 63u)) & 1ull) atomicOr(&S.flegal[o], 1ull << a);
            }
            if (sum >> 15) atomicOr(&S.allwin[o], 1ull << a);
        };
        for (;;) {
            if (kSkip & 2) break;
            int j = 0;
            if (lane == 0) j = atomicAdd(&S.job, 1);
            j = __builtin_amdgcn_readfirstlane(j);
            if (j >= jslow + jfast + jitem) break;
            if (j < jslow) {
                const int g = j * kTile + lane;
                if (g < nslow) {
                    const uint32_t pair = S.pair[GreedyLds<NT, W>::kBoards * kActions - 1 - g], o = pair >> 8, a = pair & 0xFFu;
                    const Planes q{S.board[o][0], S.board[o][1], S.board[o][2]};
                    record(o, a, greedy_reply<false>(q, (int)(S.board[o][3] & 1u), S.legal[o], a));
                }
            } else if (j < jslow + jfast) {
                const int g = (j - jslow) * kTile + lane;
                if (g < nfast) {
                    const uint32_t pair = S.pair[g], o = pair >> 8, a = pair & 0xFFu;
                    const Planes q{S.board[o][0], S.board[o][1], S.board[o][2]};
                    record(o, a, greedy_reply<true>(q, (int)(S.board[o][3] & 1u), S.legal[o], a));
                }
            } else {
                const int g = (j - jslow - jfast) * kTile + lane;
                if (g < nitems) {
                    const uint32_t it = S.item[g], o = it >> 8, jr = it & 0xFFu;
                    const Planes q{S.board[o][0], S.board[o][1], S.board[o][2]};
                    const uint32_t a2 = kth_bit64(S.replies[o], jr);
                    S.undef[o][jr] = greedy_item_row(q, (int)(S.board[o][3] & 1u), S.legal[o], a2);  // (tagged: see greedy_hand_merge_tagged)
                }
            }
        }
        GBL_WAVE_STAMP(3);
        GBL_TILE_STAMP(ts, 1);
        GBL_WAVE_STAMP(4);
        pool_fence<W>();
        GBL_WAVE_STAMP(5);
    }
    GBL_TILE_STAMP(ts, 2);
    if (!owner) return GreedyResult{-1, 0ull, false};
    if (two && !(kSkip & 1)) {  // :103-157 on the owner's lane, in closed form over the candidate sets
        ReplySets r{S.threat[bi], S.allwin[bi], S.second[bi], S.block[bi], S.flegal[bi]};
        uint64_t undef[kRootItems] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
        const int nitems_b = __popcll(plan.items);
        if (plan.items) {  // the placements settled from the root: the table's (tagged) rows merged in the reference's reply order
#pragma unroll
            for (int j = 0; j < kRootItems; ++j) undef[j] = S.undef[bi][j];
            const GreedyHandSets hs = greedy_hand_merge_tagged(nitems_b, plan.resolved, undef);
            r.threat |= hs.threat;
            r.second |= hs.second;
            r.block |= hs.block;
            r.flegal |= hs.flegal;
        }
        greedy_replay_closed(h, r, [&](int a) {
            const uint32_t twin = ((h.dup >> a) & 1ull) ? (uint32_t)a - 9u : (uint32_t)a;  // twin placements share a summary
            return ((plan.resolved >> twin) & 1ull) ? greedy_hand_lookup_tagged(nitems_b, h.legal_me, undef, twin)
                                                    : (uint32_t)S.reply[bi][twin];
        });
    }
    return greedy_finish(h, prev3);
    }
}

// greedy_tile as a real function call, for the ply loop of gbl_collect_policy: inlined there, the decision's literal
// constants are hoisted out of the loop and stay live across the whole iteration (~160 VGPRs, or spills under the kernel's
// register budget); behind a call they live and die inside the callee.
template <int NT, int W>
__device__ __attribute__((noinline)) GreedyResult greedy_tile_call(GreedyLds<NT, W> &S, Planes p, int me, uint64_t mask, int depth,
                                                                   bool deep, uint32_t prev3)
{
    TileStamps ts{};
    return greedy_tile<NT, W>(S, p, me, mask, depth, deep, prev3, ts);
}

// the agent's last three actions (one per byte, 0xFF = none) from the 6 history bytes of a board, read as three 16-bit words
__device__ __forceinline__ uint32_t hist_prev3(uint32_t h0, uint32_t h1, uint32_t h2, int me)
{
    return me ? ((h1 >> 8) | (h2 << 8)) & 0x00FFFFFFu : (h0 | (h1 << 16)) & 0x00FFFFFFu;
}

// The tile of an owner wavefront of a block: tile = block * NT + wave; tiles past the end have no rows (their wavefront still
// takes part in the block's barriers).  False: the whole block lies past the end.
template <int NT>
__device__ __forceinline__ bool block_lane_setup(Lane &L, int64_t n, int64_t ntiles)
{
    const int wave = wave_index();
    if ((int64_t)blockIdx.x * NT >= ntiles) return false;
    L.tile = (int64_t)blockIdx.x * NT + (wave < NT ? wave : 0);
    L.lane = (int)(threadIdx.x & 63u);
    const int64_t left = n - L.tile * kTile;
    L.rows = (wave >= NT || left <= 0) ? 0 : left < kTile ? (int)left : kTile;
    L.valid = L.lane < L.rows;
    L.b = L.tile * kTile + L.lane;
    return true;
}

template <int NT, int W>
__global__ __launch_bounds__(64 * W) void k_greedy(const int8_t *__restrict__ state,
                                                   const int8_t *__restrict__ to_move,
                                                   const int8_t *__restrict__ mask_in,
                                                   const int8_t *__restrict__ hist, int depth,
                                                   int32_t *__restrict__ action_out, int8_t *__restrict__ cand_out,
                                                   int8_t *__restrict__ fallback_out, int64_t n, int64_t ntiles,
                                                   int8_t *__restrict__ hist_rw, int32_t *__restrict__ final_out,
                                                   uint64_t seed, uint64_t env_base, uint32_t call,
                                                   const uint32_t *__restrict__ call_dev)
{
    if (call_dev) call += *call_dev;
    // hist_rw != NULL: gbl_greedy_act -- the history is read from and appended to hist_rw, and final_out gets
    // the action the policy returns (the fallback draw included); hist is then unused.
    if (hist_rw) hist = hist_rw;
    __shared__ uint32_t s_states[NT][image_words<kCells>()];
    __shared__ uint32_t s_masks[NT][image_words<kActions>()];
    __shared__ GreedyLds<NT, W> S;
    GBL_STAMP(0);
    GBL_STAMP_REAL(0);
    Lane L;
    if (!block_lane_setup<NT>(L, n, ntiles)) return;  // the same for every thread of the workgroup
    const int wave = wave_index();
    const bool owner = wave < NT;
    uint32_t *const s_state = s_states[owner ? wave : 0], *const s_mask = s_masks[owner ? wave : 0];
    Planes p{0u, 0u, 0u};
    uint32_t prev3 = 0x00FFFFFFu, h0 = 0xFFFFu, h1 = 0xFFFFu, h2 = 0xFFFFu;
    int me = 0;
    uint64_t mask = 0;
    if (owner && L.rows > 0) {
        // per-board scalars first, branch-free from a clamped index: in flight together with the tile (see k_step);
        // the history of BOTH agents (6 bytes, 2-byte aligned), the mover picks its three below
        const int64_t bs = L.valid ? L.b : n - 1;
        const int tm = to_move[bs];
        if (hist) {
            const uint16_t *hp = reinterpret_cast<const uint16_t *>(hist + bs * 6);
            h0 = hp[0]; h1 = hp[1]; h2 = hp[2];
        }
        uint32_t r[7];
        load_state(state, s_state, L, r);
        p = planes_of(L, r);
        me = L.valid ? (tm != 0) : 0;
        if (mask_in) {
            tile_in<kActions>(mask_in + L.tile * (kTile * kActions), s_mask, L.lane, L.rows);
            wave_lds_fence();
            uint32_t d[14];
            row_load<kActions>(s_mask, L.lane, d);
            mask = mask_bits(d);
            wave_lds_fence();
        } else {
            mask = legal54(p, me);
        }
        if (!L.valid) mask = 0;
        if (hist && L.valid)  // bytes 0-2: player_1's last three actions, bytes 3-5: player_2's
            prev3 = hist_prev3(h0, h1, h2, me);
    }
    TileStamps ts{};
    const GreedyResult g = greedy_tile<NT, W>(S, p, me, mask, depth, depth > 1, prev3, ts);
    GBL_STAMP_VAL(1, ts.t[0]);
    GBL_STAMP_VAL(2, ts.t[1]);
    GBL_STAMP_VAL(3, ts.t[2]);
    if (!owner || L.rows == 0) return;
    if (cand_out && !(knob::kGreedySkip & 16)) {
        mask_to_image<true>(s_mask, L.lane, g.cands);
        wave_lds_fence();
        tile_out<kActions>(cand_out + L.tile * (kTile * kActions), s_mask, L.lane, L.rows);
    }
    if (L.valid) {
        if (action_out) action_out[L.b] = g.fallback ? -1 : g.chosen;
        if (fallback_out) fallback_out[L.b] = g.fallback ? 1 : 0;
        if (hist_rw) {
            // :211-217 with the library's sampler, then :219
            const int fin = g.fallback ? pick54(g.cands, draw32(seed, env_base + (uint64_t)L.b, call, kStreamGreedy)) : g.chosen;
            final_out[L.b] = fin;
            int8_t *hp = hist_rw + (L.b * 2 + me) * 3;
            hp[0] = (int8_t)(prev3 >> 8);
            hp[1] = (int8_t)(prev3 >> 16);
            hp[2] = (int8_t)fin;
        }
    }
    GBL_STAMP(4);
    GBL_WAVE_STAMP(11);
    GBL_STAMP_DRAIN(5);
    GBL_STAMP_FLUSH(L.tile);
}

// gbl_collect_policy: gbl_collect with a DEVICE-SIDE POLICY per side -- masked-random, or the greedy lookahead of
// GreedyGobbletPolicy.compute_action (depth 1 / 2) -- `plies` plies per launch, every ply materialised in its trajectory
// slot.  The reference plays whole games with the greedy policy on either or both sides (tutorials/GreedyAgent/
// tutorial_greedy.py:16-54: one policy object acting for both agents, the first two plies of a game drawn at random;
// greedy_policy_tianshou.py:63-84: greedy against a learner); here the decision (greedy_tile, all W wavefronts of the
// workgroup), the fallback draw (:211-217), the history append (:219), the move, winner, auto-reset and the next
// observation / mask all happen inside one launch, the block's boards living in LDS and registers between the plies.
// The owner wavefronts do everything but the shared depth-2 work.
// (Register budget: four wavefronts per SIMD = 128 VGPRs.  Left alone the compiler takes ~160 -- the ply loop keeps the
// decision's literal constants live across iterations -- which costs a wavefront of occupancy for nothing.)
template <int NT, int W>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(W > 1 && NT == 1 ? GBL_KNOB_CP_WAVES_PER_EU : 1, 8))) void k_collect_policy(
    int8_t *__restrict__ state, int8_t *__restrict__ to_move, int64_t n, int64_t ntiles, uint64_t seed, uint64_t env_base,
    const uint32_t *__restrict__ ply_dev, uint32_t ply0, uint32_t plies, int8_t *__restrict__ done, int64_t ply_stride,
    int64_t tile_stride, int32_t *__restrict__ actions_t, int8_t *__restrict__ winner_t, int8_t *__restrict__ reward_t,
    int8_t *__restrict__ done_t, int8_t *__restrict__ to_move_t, int8_t *__restrict__ mask_t, int8_t *__restrict__ obs_t,
    int32_t *__restrict__ chosen_t, int8_t *__restrict__ how_t, int8_t *__restrict__ cand_t, int8_t *__restrict__ hist,
    int policy0, int policy1, int opening_plies, int illegal_mode, int64_t *__restrict__ counters, int32_t *__restrict__ turn)
{
    __shared__ uint32_t s_states[NT][image_words<kCells>()];
    __shared__ GreedyLds<NT, W> S;
    // The two generator blocks of a board (environment stream, fallback-draw stream: four plies' words each) are parked here, not
    // held in eight registers across the decision: a ply reads back the one word of each it needs.
    __shared__ uint32_t s_draws[NT][8][kTile];
    if (ply_dev) ply0 += *ply_dev;
    Lane L;
    if (!block_lane_setup<NT>(L, n, ntiles)) return;  // the same for every thread of the workgroup
    const int wave = wave_index();
    const bool owner = wave < NT, active = owner && L.rows > 0;
    uint32_t *const s_state = s_states[owner ? wave : 0], *const s_out = S.scratch(owner ? wave : 0);
    const bool deep = policy0 > 1 || policy1 > 1;
    Planes p{0u, 0u, 0u};
    int mover = 0, dn = 0, tabs = 0;
    uint32_t hp0 = 0x00FFFFFFu, hp1 = 0x00FFFFFFu;  // the two agents' last three actions, one per byte (0xFF = none)
    uint32_t (*const draws)[kTile] = s_draws[owner ? wave : 0];
    auto park_draws = [&](uint32_t ply) {  // the blocks that serve plies 4 * (ply >> 2) ... of this board: generated once per four plies
        const Draw4 block = draw_block(seed, env_base + (uint64_t)L.b, ply);
        Draw4 fblock{{0u, 0u, 0u, 0u}};
        if (deep || policy0 > 0 || policy1 > 0) fblock = draw_block(seed, env_base + (uint64_t)L.b, ply, kStreamGreedy);
        // (word w of a block serves the ply with ply & 3 == w: draw_word's order)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            draws[w][L.lane] = block.w[w];
            draws[4 + w][L.lane] = fblock.w[w];
        }
    };
    const ImageRow row{reinterpret_cast<uint8_t *>(s_state) + L.lane * kCells};
    uint64_t legal = 0;
    uint32_t games = 0, w1 = 0, w2 = 0;
    if (active) {
        const int64_t bs = L.valid ? L.b : n - 1;
        const int tm = to_move[bs];
        if (turn) tabs = turn[bs];
        if (hist) {
            const uint16_t *hp = reinterpret_cast<const uint16_t *>(hist + bs * 6);
            const uint32_t h0 = hp[0], h1 = hp[1], h2 = hp[2];
            hp0 = hist_prev3(h0, h1, h2, 0);
            hp1 = hist_prev3(h0, h1, h2, 1);
        }
        uint32_t r[7];
        load_state(state, s_state, L, r, [&] { park_draws(ply0); });
        mover = L.valid && tm != 0;
        p = planes_of(L, r);
        legal = legal54(p, mover);
    }
    TileStamps ts{};
    for (uint32_t t = 0; t < plies; ++t) {
        const uint32_t ply = ply0 + t;
        const int pol = mover ? policy1 : policy0;
        // the greedy policy acts on this board at this ply (tutorial_greedy.py:34-49: not on a game's opening plies)
        const bool gre = active && L.valid && pol > 0 && tabs >= opening_plies;
        const uint32_t prev3 = mover ? hp1 : hp0;
        // (one tile per workgroup: behind a call, see greedy_tile_call -- 12.6 -> 11.6 us per ply at 16 384 boards, 79 -> 71 at
        // 262 144; blocks of tiles inlined: <2,8> has the registers, <4,16> exactly its 128 since round 4 -- table above policy_shape)
        GreedyResult g;
        if constexpr (NT == 1 && W > 1)  // (<4,16> inlined holds exactly its 128 VGPRs and is 5 % faster than behind the call)
            g = greedy_tile_call<NT, W>(S, p, mover, gre ? legal : 0ull, pol, deep, prev3);
        else
            g = greedy_tile<NT, W>(S, p, mover, gre ? legal : 0ull, pol, deep, prev3, ts);
        if (!active) continue;
        int action;
        {
            // :211-217 with the library's sampler on generator stream 1 (as gbl_greedy_act, keyed by the ply index)
            // (draw32(seed, board, ply, kStreamGreedy) is word ply & 3 of the stream's block for plies 4 * (ply >> 2) ...: one
            // generator call per four plies, like the environment's)
            const uint32_t wsel = draw_word_index(ply);
            const int greedy_action = g.fallback ? pick54(g.cands, draws[4 + wsel][L.lane]) : g.chosen;
            // (the masked-random pick only where some board of the tile needs one: none in greedy-vs-greedy play past the openings;
            //  the lanes past the end of a ragged tile then play their first legal move -- never an illegal one, which in TERMINATE
            //  mode would end and restart their phantom game every ply: nothing of theirs is stored or tallied, but their state
            //  stays that of a board that is being played)
            int random_action = (int)__builtin_ctzll(legal | (1ull << 63));
            if (wave_any(L.valid && !gre)) random_action = pick54(legal, draws[wsel][L.lane]);
            action = gre ? greedy_action : random_action;
            if (gre) {  // :219: the acting agent's history takes the returned action
                const uint32_t np3 = (prev3 >> 8) | (((uint32_t)action & 0xFFu) << 16);
                hp0 = mover ? hp0 : np3;
                hp1 = mover ? np3 : hp1;
            }
        }
        if (t + 1 < plies && ((ply + 1) & 3u) == 0) park_draws(ply + 1);
        const Ply y = play_ply(p, row, mover, legal, action, illegal_mode);
        dn = y.terminal ? 1 : 0;
        if (y.terminal) {  // raw_env.reset, gobblet.py:275-290
            p = Planes{0u, 0u, 0u};
            mover = 0;
            row.reset();
        }
        tabs = next_turn(tabs, y, 1);
        if (counters) {
            games += __popcll(__ballot(L.valid && y.terminal));
            w1 += __popcll(__ballot(L.valid && y.winner == 1));
            w2 += __popcll(__ballot(L.valid && y.winner == -1));
        }
        const int64_t cell = (int64_t)t * ply_stride + L.tile * tile_stride;
        if (L.valid) {
            const int64_t at = cell + L.lane;
            if (actions_t) actions_t[at] = action;
            if (winner_t) winner_t[at] = (int8_t)y.winner;
            if (reward_t) reinterpret_cast<uint16_t *>(reward_t)[at] = (uint16_t)((y.r0 & 0xFF) | ((y.r1 & 0xFF) << 8));
            if (done_t) done_t[at] = (int8_t)dn;
            if (to_move_t) to_move_t[at] = (int8_t)mover;
            if (chosen_t) chosen_t[at] = (gre && !g.fallback) ? g.chosen : -1;
            if (how_t) how_t[at] = (int8_t)(gre ? (g.fallback ? GBL_HOW_FALLBACK : GBL_HOW_GREEDY) : GBL_HOW_RANDOM);
        }
        constexpr int kPolicy = kStoreStreamDrop;
        // The lane index the output rows are staged and stored with is made opaque once per ply: everything derived from it (image
        // offsets, the `lane < REM` predicates, buffer offsets of up to eight vectors per tile) is loop-invariant, and hoisted out of
        // the ply loop it stayed live across the decision -- under the 128-VGPR budget of the <1, W> shapes that was 22 spilled
        // registers (96 B of scratch per lane and ply); recomputing it costs a few shifts and adds per ply.
        int ol = L.lane;
#ifndef GBL_HOST_EMU
        asm volatile("" : "+v"(ol));
#endif
        auto mask_rows = [&](uint64_t bits, int8_t *__restrict__ dst) {  // (store_mask / store_obs with few registers)
            mask_to_image<true>(s_out, ol, bits);
            wave_lds_fence();
            tile_out_narrow<kActions, kPolicy, 2>(dst, s_out, ol, L.rows);
            wave_lds_fence();
        };
        wave_lds_fence();
        if (cand_t) mask_rows(gre ? g.cands : 0ull, cand_t + cell * kActions);
        if (obs_t) {
            obs_image_zero(s_out, ol);
            wave_lds_fence();
            obs_scatter(s_out, ol, p, mover);
            wave_lds_fence();
            tile_out_narrow<kObs, kPolicy, 2>(obs_t + cell * kObs, s_out, ol, L.rows);
            wave_lds_fence();
        }
        legal = legal54(p, mover);  // the next mover's: stored now, the next ply's policy is handed it
        if (mask_t) mask_rows(legal, mask_t + cell * kActions);
    }
    if (!active) return;
    wave_lds_fence();  // every lane's byte patches are in the state image
    tile_out<kCells>(state + L.tile * (kTile * kCells), s_state, L.lane, L.rows);
    if (L.valid) {
        to_move[L.b] = (int8_t)mover;
        done[L.b] = (int8_t)dn;
        if (turn) turn[L.b] = tabs;
        if (hist) {
            uint16_t *hp = reinterpret_cast<uint16_t *>(hist + L.b * 6);
            hp[0] = (uint16_t)(hp0 & 0xFFFFu);
            hp[1] = (uint16_t)(((hp0 >> 16) & 0xFFu) | ((hp1 & 0xFFu) << 8));
            hp[2] = (uint16_t)((hp1 >> 8) & 0xFFFFu);
        }
    }
    if (counters && L.lane == 0) tally_flush(counters, L.tile, L.rows, plies, games, w1, w2);
}

// Run-time flags as template arguments: f(std::bool_constant<b>...).  Every combination of the flags is instantiated: a caller keeps
// out with `if constexpr` what it never launches.
template <typename F>
void with_flags(F &&f)
{
    f();
}
template <typename F, typename... B>
void with_flags(F &&f, bool b, B... rest)
{
    if (b) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// The arguments of the five collect kernels (k_collect, k_collect2, k_collect3, k_collect5, k_collect_small), in their order -- the
// first 16 dwords arrive preloaded in SGPRs (see _native.py) -- except the count of tiles or groups, which is the launch's
struct CollectArgs {
    int8_t *state, *to_move;
    int64_t n;
    uint64_t seed, env_base;
    const uint32_t *ply_dev;
    uint32_t ply0, plies;
    int8_t *done;
    int64_t ply_stride, tile_stride;
    int32_t *actions_t;
    int8_t *winner_t, *reward_t, *done_t, *to_move_t, *mask_t, *obs_t;
    int illegal_mode;
    int64_t *counters;
    int32_t *turn;
    const int32_t *first_actions;
    int8_t *first_status;
};

template <typename Kernel>
void launch_collect(Kernel kernel, int64_t ngroups, uint32_t grid, int threads, hipStream_t s, const CollectArgs &a)
{
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), 0, s, a.state, a.to_move, a.n, ngroups, a.seed, a.env_base, a.ply_dev, a.ply0,
                       a.plies, a.done, a.ply_stride, a.tile_stride, a.actions_t, a.winner_t, a.reward_t, a.done_t, a.to_move_t, a.mask_t,
                       a.obs_t, a.illegal_mode, a.counters, a.turn, a.first_actions, a.first_status);
}

// The forms of the role kernel a build carries, as collect_variant's codes 100 LA + 10 KO + MERGE: the product's are the ones
// collect_variant() can return; an experiment build carries a whole menu (gobblet_ab.h)
using SmallForms = std::integer_sequence<int, 220, 210 GBL_KNOB_SMALL_FORMS>;

template <int LA, int KO, bool MERGE>
void launch_small_form(const CollectArgs &a, hipStream_t s)
{
    const int64_t gb = kTile / LA, ngroups = (a.n + gb - 1) / gb;
    with_flags([&](auto M, auto O, auto D) {
        launch_collect(k_collect_small<M, O, D, LA, KO, MERGE>, ngroups, (uint32_t)ngroups, 64 * small_waves<M, O, KO, MERGE>(), s, a);
    }, a.mask_t != nullptr, a.obs_t != nullptr, a.ply_dev != nullptr);
}

// k_collect_small for a checked call (see gbl_collect_from) in form cfg; false: this build has no such form
template <int... CFG>
bool launch_small(std::integer_sequence<int, CFG...>, int cfg, const CollectArgs &a, hipStream_t s)
{
    return ((cfg == CFG && (launch_small_form<CFG / 100, (CFG / 10) % 10, (CFG % 10) != 0>(a, s), true)) || ...);
}

int greedy_shape(int depth, int64_t n);  // (defined with the greedy entry points below)
int policy_shape(int depth, int64_t n);

}  // namespace

// ===========================================================================================
// C-ABI

#define GBL_NEED(p, name)                                                 \
    do {                                                                  \
        if (!(p)) return fail(GBL_ERR_ARG, name " must not be NULL");     \
    } while (0)
#define GBL_ALIGNED(p, name)                                                                   \
    do {                                                                                       \
        if (off(16, p)) return fail(GBL_ERR_ALIGN, name " must be 16-byte aligned");           \
    } while (0)
#define GBL_LAUNCH_CHECK(name) /* between the launches of one entry point */                             \
    do {                                                                                                  \
        if (const hipError_t e_ = hipGetLastError(); e_ != hipSuccess) return hip_fail(e_, name);         \
    } while (0)
#define GBL_LAUNCHED(name)     \
    do {                       \
        GBL_LAUNCH_CHECK(name); \
        return GBL_OK;         \
    } while (0)

// The alignment rules of the trajectory arguments of gbl_collect_from_ex and gbl_collect_policy (after collect_error's strides).
// words_off: whether one of the 4-byte element arrays is off a 4-byte boundary, words_msg: the error that names them.
static int check_traj(const int8_t *state, const int8_t *mask_traj, const int8_t *obs_traj, const int8_t *reward_traj, bool words_off,
                      const char *words_msg, const int32_t *turn, const int64_t *counters)
{
    GBL_ALIGNED(state, "state"); GBL_ALIGNED(mask_traj, "mask_traj"); GBL_ALIGNED(obs_traj, "obs_traj");
    if (off(2, reward_traj)) return fail(GBL_ERR_ALIGN, "reward_traj must be 2-byte aligned");
    if (words_off) return fail(GBL_ERR_ALIGN, words_msg);
    if (off(4, turn)) return fail(GBL_ERR_ALIGN, "turn must be 4-byte aligned");
    if (off(128, counters)) return fail(GBL_ERR_ALIGN, "counters must be 128-byte aligned");
    return GBL_OK;
}

// The tail the nine self-play entry points share (selfplay_launch calls it once), after their own checks: the
// trajectory's strides and alignments.  T: the kernel's SearchTraj, built by the entry point from its arguments; more_words /
// words_msg: the entry's own further 4-byte array (check_traj's words) and the message that names its whole list.
static int check_search_traj(const SearchTraj &T, const int32_t *more_words, const char *words_msg, int64_t n, uint32_t plies, int64_t ply_stride,
                             int64_t tile_stride, const int8_t *state, const int32_t *turn, const int64_t *counters)
{
    if (!strides_ok(n, plies, ply_stride, tile_stride)) return fail(GBL_ERR_ARG, kStridesMessage);
    if (const int e = check_traj(state, T.mask, T.obs, T.reward, off(4, more_words, T.actions, T.value, T.nodes), words_msg, turn, counters)) return e;
    if (off(2, T.visits)) return fail(GBL_ERR_ALIGN, "visits_traj must be 2-byte aligned");
    return GBL_OK;
}

// the grid of the one-workgroup-a-board kernels: they stride over what is beyond the cap
static inline dim3 board_grid(int64_t n) { return dim3((uint32_t)std::min<int64_t>(n, 1 << 20)); }

extern "C" {

const char *gbl_last_error(void) { return g_err; }

int gbl_layout_info(int32_t out[6])
{
    if (!out) return fail(GBL_ERR_ARG, "out must not be NULL");
    out[0] = GBL_ABI_VERSION; out[1] = kCells; out[2] = kActions; out[3] = kObs; out[4] = kTile; out[5] = 16;
    return GBL_OK;
}

int gbl_reset(int8_t *state, int8_t *to_move, int8_t *done, int8_t *winner, int64_t n, void *stream)
{
    if (const char *why = reset_error(n, state, to_move, done)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if ((e = hipMemsetAsync(state, 0, (size_t)n * kCells, s)) != hipSuccess) return hip_fail(e, "gbl_reset");
    if ((e = hipMemsetAsync(to_move, 0, (size_t)n, s)) != hipSuccess) return hip_fail(e, "gbl_reset");
    if ((e = hipMemsetAsync(done, 0, (size_t)n, s)) != hipSuccess) return hip_fail(e, "gbl_reset");
    if (winner && (e = hipMemsetAsync(winner, 0, (size_t)n, s)) != hipSuccess) return hip_fail(e, "gbl_reset");
    return GBL_OK;
}

int gbl_legal_mask(const int8_t *state, const int8_t *to_move, int8_t *mask, int64_t n, void *stream)
{
    if (const char *why = legal_mask_error(n, state, to_move, mask)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state"); GBL_ALIGNED(mask, "mask");
    Geometry g = geometry(n);
    hipLaunchKernelGGL(k_legal_mask, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, state, to_move, mask, n, g.ntiles);
    GBL_LAUNCHED("gbl_legal_mask");
}

int gbl_is_legal(const int8_t *state, const int8_t *agent_index, const int32_t *actions, int8_t *out, int64_t n,
                 void *stream)
{
    if (const char *why = is_legal_error(n, state, agent_index, actions, out)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state");
    Geometry g = geometry(n);
    hipLaunchKernelGGL(k_is_legal, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, state, agent_index, actions, out, n,
                       g.ntiles);
    GBL_LAUNCHED("gbl_is_legal");
}

int gbl_play_turn(int8_t *state, const int8_t *agent_index, const int32_t *actions, int64_t n, void *stream)
{
    if (const char *why = play_turn_error(n, state, agent_index, actions)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state");
    Geometry g = geometry(n);
    hipLaunchKernelGGL(k_play_turn, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, state, agent_index, actions, n,
                       g.ntiles);
    GBL_LAUNCHED("gbl_play_turn");
}

int gbl_winner(const int8_t *state, int8_t *winner, int64_t n, void *stream)
{
    if (const char *why = winner_error(n, state, winner)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state");
    Geometry g = geometry(n);
    hipLaunchKernelGGL(k_winner, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, state, winner, n, g.ntiles);
    GBL_LAUNCHED("gbl_winner");
}

int gbl_flatboard(const int8_t *state, int8_t *flat, int64_t n, void *stream)
{
    if (const char *why = flatboard_error(n, state, flat)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state"); GBL_ALIGNED(flat, "flat");
    Geometry g = geometry(n);
    hipLaunchKernelGGL(k_flatboard, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, state, flat, n, g.ntiles);
    GBL_LAUNCHED("gbl_flatboard");
}

int gbl_covered(const int8_t *state, int8_t *cov, int64_t n, void *stream)
{
    if (const char *why = covered_error(n, state, cov)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state"); GBL_ALIGNED(cov, "cov");
    Geometry g = geometry(n);
    hipLaunchKernelGGL(k_covered, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, state, cov, n, g.ntiles);
    GBL_LAUNCHED("gbl_covered");
}

int gbl_observe(const int8_t *state, const int8_t *to_move, int agent_sel, int8_t *obs, int64_t n, void *stream)
{
    if (const char *why = observe_error(n, state, to_move, agent_sel, obs)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state"); GBL_ALIGNED(obs, "obs");
    Geometry g = geometry(n);
    hipLaunchKernelGGL(k_observe, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, state, to_move, agent_sel, obs, n,
                       g.ntiles);
    GBL_LAUNCHED("gbl_observe");
}

int gbl_pinned_alloc(int64_t bytes, void **host_ptr, void **dev_ptr)
{
    if (bytes <= 0 || !host_ptr || !dev_ptr) return fail(GBL_ERR_ARG, "gbl_pinned_alloc: bytes > 0, host_ptr and dev_ptr required");
    void *h = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&h, (size_t)bytes, hipHostMallocMapped | hipHostMallocPortable);
    if (e != hipSuccess) return hip_fail(e, "gbl_pinned_alloc");
    e = hipHostGetDevicePointer(&d, h, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(h);
        return hip_fail(e, "gbl_pinned_alloc (device pointer)");
    }
    memset(h, 0, (size_t)bytes);
    *host_ptr = h;
    *dev_ptr = d;
    return GBL_OK;
}

int gbl_pinned_free(void *host_ptr)
{
    if (!host_ptr) return GBL_OK;
    hipError_t e = hipHostFree(host_ptr);
    if (e != hipSuccess) return hip_fail(e, "gbl_pinned_free");
    return GBL_OK;
}

int gbl_block_alloc(int64_t bytes, void **dev_ptr)
{
    if (bytes <= 0 || !dev_ptr) return fail(GBL_ERR_ARG, "gbl_block_alloc: bytes > 0 and dev_ptr required");
    void *d = nullptr;
    hipError_t e = hipMalloc(&d, (size_t)bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // (an out-of-memory answer must not linger as the thread's "last error")
        return hip_fail(e, "gbl_block_alloc");
    }
    *dev_ptr = d;
    return GBL_OK;
}

int gbl_block_free(void *dev_ptr)
{
    if (!dev_ptr) return GBL_OK;
    hipError_t e = hipFree(dev_ptr);
    if (e != hipSuccess) return hip_fail(e, "gbl_block_free");
    return GBL_OK;
}

int gbl_device_memory(int64_t *free_bytes, int64_t *total_bytes)
{
    size_t f = 0, t = 0;
    hipError_t e = hipMemGetInfo(&f, &t);
    if (e != hipSuccess) return hip_fail(e, "gbl_device_memory");
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return GBL_OK;
}

int gbl_board_eval(int8_t *state, const int8_t *agent_index, const int32_t *actions, int8_t *record_out, int64_t n,
                   void *stream)
{
    if (const char *why = board_eval_error(n, state, agent_index, actions, record_out)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state"); GBL_ALIGNED(record_out, "record_out");
    if (off(4, actions)) return fail(GBL_ERR_ALIGN, "actions must be 4-byte aligned");
    Geometry g = geometry(n);
    hipLaunchKernelGGL(k_board_eval, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, state, agent_index, actions,
                       record_out, n, g.ntiles);
    GBL_LAUNCHED("gbl_board_eval");
}

int gbl_step_ex(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *actions, int8_t *winner_out,
                int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int32_t *turn, int32_t *actions_out,
                int8_t *done_out, int8_t *to_move_out, int8_t *status_out, int32_t *next_actions_out, uint64_t seed,
                uint64_t env_base, uint32_t ply, const uint32_t *ply_dev, int64_t n, int illegal_mode, int auto_reset,
                void *stream)
{
    if (const char *why = step_error(n, state, to_move, done, actions, illegal_mode)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state"); GBL_ALIGNED(mask_out, "mask_out"); GBL_ALIGNED(obs_out, "obs_out");
    if (off(2, reward_out)) return fail(GBL_ERR_ALIGN, "reward_out must be 2-byte aligned");
    if (off(4, turn)) return fail(GBL_ERR_ALIGN, "turn must be 4-byte aligned");
    if (off(4, actions)) return fail(GBL_ERR_ALIGN, "actions must be 4-byte aligned");
    if (off(4, actions_out)) return fail(GBL_ERR_ALIGN, "actions_out must be 4-byte aligned");
    if (off(4, next_actions_out)) return fail(GBL_ERR_ALIGN, "next_actions_out must be 4-byte aligned");
    Geometry g = geometry(n, kStepWaves);
    hipStream_t s = (hipStream_t)stream;
    auto_reset = auto_reset != 0;
    const int nt = nt_policy(n);
    const bool ext = actions_out || done_out || to_move_out || status_out || next_actions_out;
    const StepExt X{actions_out, done_out, to_move_out, status_out, next_actions_out, seed, env_base, ply_dev, ply};
    with_flags([&](auto M, auto O, auto NT3, auto EXT) {
        hipLaunchKernelGGL((k_step<M, O, NT3 ? 3 : 1, EXT>), dim3(g.grid), dim3(64 * kStepWaves), 0, s, state, to_move, done, actions, n,
                           g.ntiles, illegal_mode, auto_reset, winner_out, reward_out, mask_out, obs_out, turn, X);
    }, mask_out != nullptr, obs_out != nullptr, nt == 3, ext);
    GBL_LAUNCHED("gbl_step");
}

int gbl_sample_at(const int8_t *mask, int32_t *actions, int64_t n, uint64_t seed, uint64_t env_base, uint32_t ply,
                  const uint32_t *ply_dev, void *stream)
{
    if (const char *why = sample_error(n, mask, actions)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(mask, "mask");
    Geometry g = geometry(n);
    hipLaunchKernelGGL(k_sample, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, mask, actions, n, g.ntiles, seed,
                       env_base, ply, ply_dev);
    GBL_LAUNCHED("gbl_sample");
}

int gbl_counter_add(uint32_t *counter, uint32_t by, void *stream)
{
    if (!counter) return fail(GBL_ERR_ARG, "counter must not be NULL");
    hipLaunchKernelGGL(k_counter_add, dim3(1), dim3(1), 0, (hipStream_t)stream, counter, by);
    GBL_LAUNCHED("gbl_counter_add");
}

int gbl_rollout_at(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_out, int8_t *winner_out,
                   int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int64_t n, uint64_t seed, uint64_t env_base,
                   uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int illegal_mode, int64_t *counters,
                   int32_t *turn, void *stream)
{
    if (const char *why = rollout_error(n, state, to_move, done, illegal_mode)) return fail(GBL_ERR_ARG, why);
    if (n == 0 || plies == 0) return GBL_OK;
    GBL_ALIGNED(state, "state"); GBL_ALIGNED(mask_out, "mask_out"); GBL_ALIGNED(obs_out, "obs_out");
    if (off(2, reward_out)) return fail(GBL_ERR_ALIGN, "reward_out must be 2-byte aligned");
    if (off(128, counters)) return fail(GBL_ERR_ALIGN, "counters must be 128-byte aligned");
    if (off(4, turn)) return fail(GBL_ERR_ALIGN, "turn must be 4-byte aligned");
    if (off(4, actions_out)) return fail(GBL_ERR_ALIGN, "actions_out must be 4-byte aligned");
    Geometry g = geometry(n, kStepWaves);
    hipStream_t s = (hipStream_t)stream;
    const int nt = nt_policy(n);
    with_flags([&](auto M, auto O, auto NT3, auto D, auto ONE) {
        hipLaunchKernelGGL((k_rollout<M, O, NT3 ? 3 : 1, D, ONE>), dim3(g.grid), dim3(64 * kStepWaves), 0, s, state, to_move, n, g.ntiles,
                           seed, env_base, ply_dev, ply0, plies, done, actions_out, winner_out, reward_out, mask_out, obs_out, illegal_mode,
                           counters, turn);
    }, mask_out != nullptr, obs_out != nullptr, nt == 3, ply_dev != nullptr, plies == 1);
    GBL_LAUNCHED("gbl_rollout");  // (also gbl_rollout_at)
}

int gbl_collect_from_ex(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *first_actions, int8_t *first_status,
                        int32_t *actions_traj, int8_t *winner_traj, int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj,
                        int8_t *mask_traj, int8_t *obs_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed,
                        uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int illegal_mode,
                        int64_t *counters, int32_t *turn, void *stream)
{
    if (n > 0 && off(4, first_actions)) return fail(GBL_ERR_ALIGN, "first_actions must be 4-byte aligned");  // (in front of every rule but n's)
    if (const char *why = collect_error(n, first_actions, first_status, state, to_move, done, illegal_mode, plies, ply_stride, tile_stride))
        return fail(GBL_ERR_ARG, why);
    if (n == 0 || plies == 0) return GBL_OK;
    if (const int e = check_traj(state, mask_traj, obs_traj, reward_traj, off(4, actions_traj), "actions_traj must be 4-byte aligned", turn, counters))
        return e;
    const Geometry g = geometry(n);
    const hipStream_t s = (hipStream_t)stream;
    const int variant = collect_variant(n, plies, mask_traj != nullptr, obs_traj != nullptr);
    const CollectArgs a{state,       to_move,     n,         seed,         env_base,  ply_dev,  ply0,     plies,
                        done,        ply_stride,  tile_stride, actions_traj, winner_traj, reward_traj, done_traj, to_move_traj,
                        mask_traj,   obs_traj,    illegal_mode, counters,    turn,      first_actions, first_status};
    if (GBL_COLLECT_IS_ROLES(variant)) {
        if (!launch_small(SmallForms{}, variant - GBL_COLLECT_ROLES(0, 0, 0), a, s))
            return fail(GBL_ERR_ARG, "gbl_collect: this build has no such form of the role kernel");
        GBL_LAUNCHED("gbl_collect");
    }
    with_flags([&](auto M, auto O, auto D) {
        if (variant == GBL_COLLECT_TRIO) {
            if constexpr (M || O) {  // (collect_variant sends no launch without rows to k_collect3)
                with_flags([&](auto H) { launch_collect(k_collect3<M, O, D, H>, g.ntiles, (uint32_t)g.ntiles, 64 * (1 + M + O), s, a); },
                           g.ntiles <= kTrioHandMaxTiles);
            }
        } else if (variant == GBL_COLLECT_GROUP32) {
            const int64_t ngroups = (n + kGroupBoards - 1) / kGroupBoards;
            launch_collect(k_collect5<O, D>, ngroups, (uint32_t)ngroups, 64 * (O ? 4 : 2), s, a);
        } else if (variant == GBL_COLLECT_PAIR) {
            launch_collect(k_collect2<M, O, D>, g.ntiles, (uint32_t)g.ntiles, 128, s, a);
        } else if constexpr (knob::kForcedCollectNt < 0) {
            launch_collect(k_collect<M, O, D, true>, g.ntiles, g.grid, 64, s, a);
        } else {  // (the plain-store instantiation of k_collect exists in experiment builds only)
            with_flags([&](auto NT) { launch_collect(k_collect<M, O, D, NT>, g.ntiles, g.grid, 64, s, a); }, variant != GBL_COLLECT_CACHED);
        }
    }, mask_traj != nullptr, obs_traj != nullptr, ply_dev != nullptr);
    GBL_LAUNCHED("gbl_collect");
}

int gbl_collect_policy(int8_t *state, int8_t *to_move, int8_t *done, int8_t *hist, int32_t *actions_traj,
                       int8_t *winner_traj, int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj,
                       int8_t *obs_traj, int32_t *chosen_traj, int8_t *how_traj, int8_t *cand_traj, int64_t n,
                       int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                       const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, int opening_plies,
                       int illegal_mode, int64_t *counters, int32_t *turn, void *stream)
{
    if (const char *why = collect_policy_error(n, state, to_move, done, illegal_mode, policy0, policy1, opening_plies, turn != nullptr, plies,
                                               ply_stride, tile_stride))
        return fail(GBL_ERR_ARG, why);
    if (n == 0 || plies == 0) return GBL_OK;
    if (const int e = check_traj(state, mask_traj, obs_traj, reward_traj, off(4, actions_traj, chosen_traj),
                                 "actions_traj / chosen_traj must be 4-byte aligned", turn, counters))
        return e;
    GBL_ALIGNED(cand_traj, "cand_traj");
    if (off(2, hist)) return fail(GBL_ERR_ALIGN, "hist must be 2-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int depth = policy0 > policy1 ? policy0 : policy1;
    const int shape = policy_shape(depth, n);
#define GBL_CP(NT, W)                                                                                                      \
    do {                                                                                                                   \
        const Geometry g = block_geometry(n, NT);                                                                          \
        hipLaunchKernelGGL((k_collect_policy<NT, W>), dim3(g.grid), dim3(64 * W), 0, s, state, to_move, n, g.ntiles, seed,  \
                           env_base, ply_dev, ply0, plies, done, ply_stride, tile_stride, actions_traj, winner_traj,       \
                           reward_traj, done_traj, to_move_traj, mask_traj, obs_traj, chosen_traj, how_traj, cand_traj,    \
                           hist, policy0, policy1, opening_plies, illegal_mode, counters, turn);                           \
    } while (0)
    // (the product build instantiates the shapes policy_shape() can return; an A/B build the one it forces as well)
    if (shape == 56) GBL_CP(4, 16);
    else if (shape == 26) GBL_CP(1, 16);
    else if (shape == 28) GBL_CP(2, 8);
    else if (shape == 14) GBL_CP(1, 4);
    GBL_KNOB_CP_SHAPES
    else GBL_CP(1, 1);
#undef GBL_CP
    GBL_LAUNCHED("gbl_collect_policy");
}

int gbl_collect_variant(int64_t n, uint32_t plies, int with_mask, int with_obs)
{
    if (n < 0) return fail(GBL_ERR_ARG, "n < 0");
    return collect_variant(n, plies, with_mask != 0, with_obs != 0);
}

int gbl_placement_probe(void *a, int64_t a_bytes, void *b, int64_t b_bytes, int64_t slot_boards, int plies, float *us_both,
                        float *us_a, float *us_b, void *stream)
{
    GBL_NEED(a, "a"); GBL_NEED(b, "b"); GBL_NEED(us_both, "us_both"); GBL_NEED(us_a, "us_a"); GBL_NEED(us_b, "us_b");
    if (off(128, a, b)) return fail(GBL_ERR_ALIGN, "a and b must be 128-byte aligned");
    int kPlies = 4;
    int64_t tiles;
    if (slot_boards > 0) {  // the geometry of a time-major trajectory: `plies` slots of slot_boards boards
        if (plies < 1 || (slot_boards & 127)) return fail(GBL_ERR_ARG, "slot_boards: a multiple of 128 boards; plies >= 1");
        kPlies = plies;
        tiles = slot_boards / kTile;
        if (a_bytes < (int64_t)plies * slot_boards * kObs || b_bytes < (int64_t)plies * slot_boards * kActions)
            return fail(GBL_ERR_ARG, "buffers smaller than plies x slot_boards rows");
    } else {
        // an even number of tiles per slot: every slot of both arrays then starts on a 128-byte line
        tiles = std::min(a_bytes / ((int64_t)kPlies * kTile * kObs), b_bytes / ((int64_t)kPlies * kTile * kActions)) & ~(int64_t)1;
    }
    if (tiles < 2) return fail(GBL_ERR_ARG, "buffers too small to probe (a: 4 x 7488 bytes per tile, b: 4 x 3456)");
    if (tiles > 0x7fffffff) return fail(GBL_ERR_ARG, "buffers too large to probe in one launch");
    hipStream_t s = (hipStream_t)stream;
    int8_t *pa = static_cast<int8_t *>(a), *pb = static_cast<int8_t *>(b);
    auto launch = [&](int which) {
        if (which == 0) hipLaunchKernelGGL((k_probe<true, true>), dim3((uint32_t)tiles), dim3(64), 0, s, pa, pb, tiles, kPlies);
        else if (which == 1) hipLaunchKernelGGL((k_probe<true, false>), dim3((uint32_t)tiles), dim3(64), 0, s, pa, pb, tiles, kPlies);
        else hipLaunchKernelGGL((k_probe<false, true>), dim3((uint32_t)tiles), dim3(64), 0, s, pa, pb, tiles, kPlies);
        return hipGetLastError();
    };
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    // a probe often runs on an idle device (the caller has just allocated memory): bring the clocks up first, then
    // time the three variants back to back, several rounds, and keep each one's best
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = launch(0);
    float best[3] = {0.f, 0.f, 0.f};
    constexpr int kRounds = 4;
    for (int round = 0; round < kRounds && e == hipSuccess; ++round) {
        e = hipEventRecord(ev[0], s);
        for (int which = 1; which <= 3 && e == hipSuccess; ++which) {  // a alone, b alone, both
            e = launch(which % 3);
            if (e == hipSuccess) e = hipEventRecord(ev[which], s);
        }
        if (e == hipSuccess) e = hipEventSynchronize(ev[3]);
        for (int which = 1; which <= 3 && e == hipSuccess; ++which) {
            float ms = 0.f;
            e = hipEventElapsedTime(&ms, ev[which - 1], ev[which]);
            float &slot = best[which % 3];
            if (round == 0 || ms < slot) slot = ms;
        }
    }
    for (int i = 0; i < 4; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    if (e != hipSuccess) return hip_fail(e, "gbl_placement_probe");
    *us_both = best[0] * 1e3f;
    *us_a = best[1] * 1e3f;
    *us_b = best[2] * 1e3f;
    return GBL_OK;
}

int gbl_decode_obs(const int8_t *obs, int8_t *state, int8_t *to_move, int64_t n, void *stream)
{
    if (const char *why = decode_obs_error(n, obs, state, to_move)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(obs, "obs"); GBL_ALIGNED(state, "state");
    Geometry g = geometry(n);
    hipLaunchKernelGGL(k_decode_obs, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, obs, state, to_move, n, g.ntiles);
    GBL_LAUNCHED("gbl_decode_obs");
}

int gbl_validate(const int8_t *state, int8_t *flags, int64_t n, void *stream)
{
    if (const char *why = validate_error(n, state, flags)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state");
    Geometry g = geometry(n);
    hipLaunchKernelGGL(k_validate, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, state, flags, n, g.ntiles);
    GBL_LAUNCHED("gbl_validate");
}

namespace {
// The shape of the greedy kernels' workgroups (see GreedyLds), as a code: 11 = <1,1>, 14 = <1,4>, 18 = <1,8>, 26 = <1,16>,
// 28 = <2,8>, 48 = <4,8>, 56 = <4,16>.
// Round 1 (one tile per workgroup; scripts/bench_greedy.py, 65 536 / 262 144 / 2^20 boards): 1 wavefront 49 / 155 / 518 us,
// 2: 43 / 139 / 487, 4: 41 / 121 / 451, 8: 40 / 136 / 520, 16: 50 / 176 / 679.  Round 2 (scripts/ab_greedy.py, in-process):
// eight wavefronts shorten a lone tile's serial chain -- 4 096 / 16 384 boards 11.2 / 11.4 -> 10.0 / 10.2 us -- and lose
// 2-4 % beyond 131 072 boards.  Round 3 (ab_greedy.py / ab_policy_collect.py): what decides is how many
// wavefronts a SIMD has to issue from WHILE THE PAIRS ARE EVALUATED (this code needs four to hide its own LDS round trips
// and dependency chains) against how many sit idle through the owners' phases:
//   gbl_greedy, us (with the two-form pair evaluation, r03 shapes sweep):
//                          4 096   16 384   32 768   49 152   65 536   98 304   131 072   196 608   262 144    2^20
//     <1,4>                  9.4     9.4      11.5     13.0     14.4     20.5      25.8      34.7      43.6     152
//     <1,8>                  8.7     8.9      11.2     13.0     17.3     24.4      31.2      43.3      55.0     201
//     <1,16>                 8.9     9.0      14.8     20.6     26.2       -         -         -         -        -
//     <2,8>                 10.1    10.0      10.2     13.8     13.9     20.4      24.6      35.1      45.5     167
//     <4,8>                 12.7    12.8      12.9     13.1     13.2     24.1      25.1      36.4      48.1     182
//     <4,16>                11.7    11.5      11.5     11.9     12.0     21.8      22.7      32.8      43.1     165
// (<1,16>: one workgroup per CU up to 256 tiles; <4,16>: four owners, four helpers, four wavefronts for the nonplain sets and
// four more that only evaluate -- 16 wavefronts per CU for one GENERATION of tiles, 65 536 boards; a launch of 1.5 generations
// takes as long as one of two, so between generations the smallest workgroups take over, and beyond four they win anyway.)
[[maybe_unused]] static bool whole_generations(int64_t n)  // the last generation of 65 536-board blocks is at least 80 % full
{
    const int64_t gens = (n + 65535) / 65536;
    return n * 5 >= gens * 65536 * 4;
}

int greedy_shape(int depth, int64_t n)
{
    if (knob::kForcedGreedyShape) return depth == 1 ? 11 : knob::kForcedGreedyShape;
    // (round 5, scripts/ab_greedy.py: at 262 144 boards <1,4> 39.8 us against <4,16>'s 40.8 since the depth-1 walk is a closed form)
    return depth == 1 ? 11 : n <= 16384 ? 26 : n <= 32768 ? 28 : n <= 65536 ? 56 : n <= 196608 && whole_generations(n) ? 56 : 14;
}

// ... and of gbl_collect_policy's, whose ply loop keeps more registers live: blocks of tiles only where they stay inlined
// within the register file.  us per self-play ply (r03 shapes sweep):
//                          4 096   16 384   32 768   65 536   131 072   262 144
//     <1,4>                 11.5    11.7      13.8     17.2      32.7      62.4
//     <1,8>                 10.6    10.8      13.3     25.3      49.4      96.7
//     <1,16>                10.6    10.7      21.0     41.8        -         -
//     <2,8>                 11.2    11.0      11.2     22.4      44.2      87.8
//     <4,8>                 15.0    14.9      15.0     15.5      30.5      60.4
//     <4,16> (behind a call) 16.5   16.7      16.7     16.9      33.3      66.2
// Round 4 (scripts/ab_policy_collect.py; the wave index a scalar, the output rows' lane index opaque per ply, the two generator
// blocks parked in LDS: <4,8> 209 -> 132 VGPRs, and <4,16> fits its 128 INLINED without a spill):
//                                            32 768   65 536   131 072   262 144
//     <2,8>  / <4,8>  (round 3's choice)       11.1     15.0      29.9      59.4
//     the same after the register work         10.9     14.7      29.0      57.7
//     <4,16> behind a call                     13.2     13.5      26.6      52.7
//     <4,16> inlined                           12.6     12.9      25.2      49.9
int policy_shape(int depth, int64_t n)
{
    if (knob::kForcedGreedyShape) return depth <= 1 ? 11 : knob::kForcedGreedyShape;
    return depth <= 1 ? 11 : n <= 16384 ? 26 : n <= 32768 ? 28 : n <= 65536 ? 56 : n <= 262144 && whole_generations(n) ? 56 : 14;
}

void launch_greedy(int shape, int64_t n, hipStream_t stream, const int8_t *state, const int8_t *to_move,
                   const int8_t *mask, const int8_t *hist, int depth, int32_t *action_out, int8_t *cand_mask_out,
                   int8_t *fallback_out, int8_t *hist_rw, int32_t *final_out, uint64_t seed,
                   uint64_t env_base, uint32_t call, const uint32_t *call_dev = nullptr)
{
#define GBL_GREEDY(NT, W)                                                                                              \
    do {                                                                                                               \
        const Geometry g = block_geometry(n, NT);                                                                      \
        hipLaunchKernelGGL((k_greedy<NT, W>), dim3(g.grid), dim3(64 * W), 0, stream, state, to_move, mask, hist, depth, \
                           action_out, cand_mask_out, fallback_out, n, g.ntiles, hist_rw, final_out, seed, env_base,   \
                           call, call_dev);                                                                            \
    } while (0)
    // (the product build instantiates the shapes greedy_shape() can return; an A/B build the one it forces as well)
    if (shape == 56) GBL_GREEDY(4, 16);
    else if (shape == 28) GBL_GREEDY(2, 8);
    else if (shape == 26) GBL_GREEDY(1, 16);
    else if (shape == 14) GBL_GREEDY(1, 4);
    GBL_KNOB_GREEDY_SHAPES
    else GBL_GREEDY(1, 1);
#undef GBL_GREEDY
}
}  // namespace

int gbl_greedy(const int8_t *state, const int8_t *to_move, const int8_t *mask, const int8_t *hist, int depth,
               int32_t *action_out, int8_t *cand_mask_out, int8_t *fallback_out, int64_t n, void *stream)
{
    if (const char *why = greedy_error(n, state, to_move, action_out, depth)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state"); GBL_ALIGNED(mask, "mask"); GBL_ALIGNED(cand_mask_out, "cand_mask_out");
    if (off(2, hist)) return fail(GBL_ERR_ALIGN, "hist must be 2-byte aligned");
    launch_greedy(greedy_shape(depth, n), n, (hipStream_t)stream, state, to_move, mask, hist, depth, action_out,
                  cand_mask_out, fallback_out, nullptr, nullptr, 0, 0, 0);
    GBL_LAUNCHED("gbl_greedy");
}

int gbl_greedy_act_at(const int8_t *state, const int8_t *to_move, const int8_t *mask, int8_t *hist, int depth,
                      uint64_t seed, uint64_t env_base, uint32_t call, const uint32_t *call_dev, int32_t *action_out,
                      int32_t *chosen_out, int8_t *cand_mask_out, int8_t *fallback_out, int64_t n, void *stream)
{
    if (const char *why = greedy_act_error(n, state, to_move, hist, action_out, depth)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state, "state"); GBL_ALIGNED(mask, "mask"); GBL_ALIGNED(cand_mask_out, "cand_mask_out");
    if (off(2, hist)) return fail(GBL_ERR_ALIGN, "hist must be 2-byte aligned");
    launch_greedy(greedy_shape(depth, n), n, (hipStream_t)stream, state, to_move, mask, nullptr, depth, chosen_out,
                  cand_mask_out, fallback_out, hist, action_out, seed, env_base, call, call_dev);
    GBL_LAUNCHED("gbl_greedy_act");
}

int gbl_playout_values(const int8_t *state, const int8_t *to_move, const int8_t *mask, int playouts, int max_plies,
                       uint64_t seed, uint64_t env_base, uint32_t call, int32_t *wins_out, int32_t *losses_out,
                       int32_t *action_out, int32_t *plies_out, int64_t n, void *stream)
{
    if (const char *why = playout_values_error(playouts, max_plies, call, env_base, n, state, to_move)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    if (off(4, wins_out, losses_out, action_out, plies_out))
        return fail(GBL_ERR_ALIGN, "wins_out / losses_out / action_out / plies_out must be 4-byte aligned");
    const uint32_t K = (uint32_t)playouts;
    const uint64_t kinv = ((1ull << 32) + K - 1) / K;
    const dim3 grid = board_grid(n);
    const hipStream_t s = (hipStream_t)stream;
#define GBL_PLAYOUT(W)                                                                                                          \
    hipLaunchKernelGGL((k_playout<W>), grid, dim3(64 * W), 0, s, state, to_move, mask, wins_out, losses_out, action_out, plies_out, \
                       n, seed, env_base, call, K, kinv, (uint32_t)max_plies)
    switch (playout_waves(n, playouts)) {
    case 8: GBL_PLAYOUT(8); break;
    case 4: GBL_PLAYOUT(4); break;
    case 2: GBL_PLAYOUT(2); break;
    default: GBL_PLAYOUT(1); break;
    }
#undef GBL_PLAYOUT
    GBL_LAUNCHED("gbl_playout_values");
}

int gbl_tree_search(const int8_t *state, const int8_t *to_move, const int8_t *mask, int iterations, int playouts, int max_plies,
                    int explore, uint64_t seed, uint64_t env_base, uint32_t call, int32_t *visits_out, int32_t *wins_out,
                    int32_t *losses_out, int32_t *action_out, int32_t *nodes_out, int32_t *plies_out, int64_t n, void *stream)
{
    if (const char *why = tree_search_error(iterations, playouts, max_plies, explore, call, env_base, n, state, to_move))
        return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    if (off(4, visits_out, wins_out, losses_out, action_out, nodes_out, plies_out))
        return fail(GBL_ERR_ALIGN, "visits_out / wins_out / losses_out / action_out / nodes_out / plies_out must be 4-byte aligned");
    const dim3 grid = board_grid(n);
    const size_t lds = sizeof(TreeNode) * ((size_t)iterations + 1);  // the tree: one node per iteration and the root
    const hipStream_t s = (hipStream_t)stream;
#define GBL_TREE(W)                                                                                                               \
    hipLaunchKernelGGL((k_tree<W>), grid, dim3(64 * W), lds, s, state, to_move, mask, visits_out, wins_out, losses_out, action_out, \
                       nodes_out, plies_out, n, seed, env_base, call, (uint32_t)iterations, (uint32_t)playouts, (uint32_t)max_plies, \
                       (uint32_t)explore)
    switch (tree_waves(n, playouts)) {
    case 4: GBL_TREE(4); break;
    case 2: GBL_TREE(2); break;
    default: GBL_TREE(1); break;
    }
#undef GBL_TREE
    GBL_LAUNCHED("gbl_tree_search");
}

int gbl_solve(const int8_t *state, const int8_t *to_move, const int8_t *mask, int depth, int8_t *outcome_out, int8_t *value_out,
              int32_t *action_out, int64_t n, void *stream)
{
    int code = 0;
    if (const char *why = solve_error(depth, n, state, to_move, action_out, code)) return fail(code ? GBL_ERR_ALIGN : GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    hipLaunchKernelGGL((k_solve<knob::kSolveDeal>), board_grid(n), dim3(64), 0, (hipStream_t)stream, state, to_move, mask, outcome_out, value_out,
                       action_out, n, depth);
    GBL_LAUNCHED("gbl_solve");
}

// gbl_evaluator as the kernels take it, after the checks both entry points share; 0, or the error
static int eval_net_of(const gbl_evaluator *ev, EvalNet &net)
{
    if (const char *why = evaluator_pointers_error(ev)) return fail(GBL_ERR_ARG, why);
    if (off(16, ev->w1, ev->b1, ev->w2, ev->b2)) return fail(GBL_ERR_ALIGN, "the evaluator's w1 / b1 / w2 / b2 must be 16-byte aligned");
    net = EvalNet{ev->w1, ev->b1, ev->w2, ev->b2, ev->hidden, ev->shift1, ev->shift_p, ev->shift_v};
    return GBL_OK;
}

int gbl_evaluate(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, uint8_t *priors_out,
                 int32_t *value_out, int32_t *logits_out, int64_t n, void *stream)
{
    if (const char *why = evaluate_error(ev, n, state, to_move, priors_out, value_out)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    EvalNet net;
    if (const int e = eval_net_of(ev, net)) return e;
    if (off(4, value_out, logits_out)) return fail(GBL_ERR_ALIGN, "value_out / logits_out must be 4-byte aligned");
    hipLaunchKernelGGL(k_evaluate, board_grid(n), dim3(64), 0, (hipStream_t)stream, state, to_move, mask, net, priors_out, value_out,
                       logits_out, n);
    GBL_LAUNCHED("gbl_evaluate");
}

// gbl_tree_search_eval and gbl_tree_search_eval_noise: one kernel in two instantiations, with and without the noise's code
static int tree_search_eval_launch(const char *name, const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev,
                                   int iterations, int explore, int noise, uint64_t seed, uint64_t env_base, uint32_t call,
                                   int32_t *visits_out, int32_t *wins_out, int32_t *losses_out, int32_t *action_out, int32_t *nodes_out,
                                   int32_t *root_value_out, uint8_t *root_priors_out, uint8_t *root_mixed_out, int64_t n, void *stream)
{
    if (const char *why = tree_search_eval_error(ev, iterations, explore, n, state, to_move)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    EvalNet net;
    if (const int e = eval_net_of(ev, net)) return e;
    if (off(4, visits_out, wins_out, losses_out, action_out, nodes_out, root_value_out))
        return fail(GBL_ERR_ALIGN, "visits_out / wins_out / losses_out / action_out / nodes_out / root_value_out must be 4-byte aligned");
    // the tree: a node and a prior row per iteration, and the root's (36.9 KB at 512 iterations: below the 64 KB a kernel gets unasked)
    const size_t lds = (sizeof(TreeNode) + kEvalOutputs) * ((size_t)iterations + 1);
    // (k_tree_eval<false> is the kernel without the noise's code; a caller who asks for root_mixed_out at weight 0 gets the <true> one)
#define GBL_TE(NOISE)                                                                                                                   \
    hipLaunchKernelGGL(k_tree_eval<NOISE>, board_grid(n), dim3(64), lds, (hipStream_t)stream, state, to_move, mask, net, visits_out,    \
                       wins_out, losses_out, action_out, nodes_out, root_value_out, root_priors_out, n, (uint32_t)iterations,           \
                       (uint32_t)explore, root_mixed_out, (uint32_t)noise, seed, env_base, call, GumbelOutputs{})
    if (noise || root_mixed_out)
        GBL_TE(true);
    else
        GBL_TE(false);
#undef GBL_TE
    GBL_LAUNCHED(name);
}

int gbl_tree_search_eval(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                         int explore, int32_t *visits_out, int32_t *wins_out, int32_t *losses_out, int32_t *action_out,
                         int32_t *nodes_out, int32_t *root_value_out, uint8_t *root_priors_out, int64_t n, void *stream)
{
    return tree_search_eval_launch("gbl_tree_search_eval", state, to_move, mask, ev, iterations, explore, 0, 0, 0, 0, visits_out, wins_out,
                                   losses_out, action_out, nodes_out, root_value_out, root_priors_out, nullptr, n, stream);
}

int gbl_tree_search_eval_noise(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                               int explore, int noise, uint64_t seed, uint64_t env_base, uint32_t call, int32_t *visits_out,
                               int32_t *wins_out, int32_t *losses_out, int32_t *action_out, int32_t *nodes_out, int32_t *root_value_out,
                               uint8_t *root_priors_out, uint8_t *root_mixed_out, int64_t n, void *stream)
{
    if (const char *why = tree_search_noise_error(noise, call, env_base, n)) return fail(GBL_ERR_ARG, why);
    return tree_search_eval_launch("gbl_tree_search_eval_noise", state, to_move, mask, ev, iterations, explore, noise, seed, env_base, call,
                                   visits_out, wins_out, losses_out, action_out, nodes_out, root_value_out, root_priors_out, root_mixed_out,
                                   n, stream);
}

// gbl_tree_search_gumbel: k_tree_eval's instantiation with the Gumbel root rule and without the noise's code
int gbl_tree_search_gumbel(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                           int explore, int considered, int gumbel_noise, int visit_offset, int scale, uint64_t seed, uint64_t env_base,
                           uint32_t call, int32_t *visits_out, int32_t *wins_out, int32_t *losses_out, int32_t *action_out,
                           int32_t *nodes_out, int32_t *root_value_out, uint8_t *root_priors_out, uint8_t *target_out, int16_t *gumbel_out,
                           int64_t n, void *stream)
{
    if (const char *why = tree_search_gumbel_error(ev, iterations, explore, considered, gumbel_noise, visit_offset, scale, call, env_base, n,
                                                   state, to_move))
        return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    EvalNet net;
    if (const int e = eval_net_of(ev, net)) return e;
    if (off(4, visits_out, wins_out, losses_out, action_out, nodes_out, root_value_out))
        return fail(GBL_ERR_ALIGN, "visits_out / wins_out / losses_out / action_out / nodes_out / root_value_out must be 4-byte aligned");
    if (off(2, gumbel_out)) return fail(GBL_ERR_ALIGN, "gumbel_out must be 2-byte aligned");
    const size_t lds = (sizeof(TreeNode) + kEvalOutputs) * ((size_t)iterations + 1);  // (the tree of gbl_tree_search_eval: the rule adds none)
    hipLaunchKernelGGL((k_tree_eval<false, true>), board_grid(n), dim3(64), lds, (hipStream_t)stream, state, to_move, mask, net, visits_out,
                       wins_out, losses_out, action_out, nodes_out, root_value_out, root_priors_out, n, (uint32_t)iterations,
                       (uint32_t)explore, (uint8_t *)nullptr, 0u, seed, env_base, call,
                       GumbelOutputs{target_out, gumbel_out,
                                     GumbelArgs{(uint32_t)considered, (uint32_t)gumbel_noise, (uint32_t)visit_offset, (uint32_t)scale}});
    GBL_LAUNCHED("gbl_tree_search_gumbel");
}

// The self-play entry points (gbl_collect_search and its _eval, _solve, _noise, _cap, _gumbel and _tb, gbl_collect_gumbel_solve and gbl_collect_gumbel_tb) between the C ABI and the launch: the checks both flavours share (selfplay_prologue), the
// evaluators as the kernels take them, the trajectory's strides and alignments, the grid, the tree's LDS and the entry's own kernel.
static int selfplay_launch(const char *name, const SelfplayCall<gbl_evaluator> &c, void *stream)
{
    EvalNet nets[2] = {};  // (a RANDOM side's stays empty: the kernel never reads it)
    int most = 0;          // the larger tree of the sides that search
    const int go = selfplay_prologue(c, most, [](const char *why) { return fail(GBL_ERR_ARG, why); },
                                     [&](int m) { return eval_net_of(c.ev[m], nets[m]); });
    if (go <= 0) return go;
    const bool uct = c.run == kRunSearch;
    const SelfplayTraj &t = c.traj;
    const SearchTraj T{t.actions, t.winner, t.reward, t.done, t.to_move, t.mask, t.obs, t.visits, t.value, t.nodes, t.how, t.mover};
    if (const int e = check_search_traj(T, t.root_value,
                                        uct ? "actions_traj / value_traj / nodes_traj must be 4-byte aligned"
                                            : "actions_traj / value_traj / nodes_traj / root_value_traj must be 4-byte aligned",
                                        c.n, c.plies, c.ply_stride, c.tile_stride, c.state, c.turn, c.counters))
        return e;
    const bool reads_table = selfplay_reads_table(c);
    if (reads_table) GBL_ALIGNED(c.aux, "aux");
    const dim3 grid((uint32_t)std::min<int64_t>(c.n, 1 << 20));
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t its0 = (uint32_t)c.iterations[0], its1 = (uint32_t)c.iterations[1], explore = (uint32_t)c.explore;
    // the tree: one node per iteration and the root; with an evaluator a prior row beside each (36.9 KB at 512 iterations, as
    // gbl_tree_search_eval; the solver's arrays are static LDS beside it)
    const size_t lds = (sizeof(TreeNode) + (uct ? 0 : kEvalOutputs)) * ((size_t)most + 1);
    // gbl_collect_gumbel_solve: a call with a Gumbel side and a guarded side runs its own kernel; with no Gumbel side it is
    // gbl_collect_search_solve's launch below, and with no guarded side and neither of the guard's arrays to fill it is
    // gbl_collect_search_gumbel's (k_collect_eval writes no outcome row: a call that wants the GBL_SOLVE_NONE rows keeps the kernel that does)
    const bool guarded = (c.policy[0] == GBL_POLICY_EVAL_TREE && c.solve_depth[0] > 0) || (c.policy[1] == GBL_POLICY_EVAL_TREE && c.solve_depth[1] > 0);
    const bool rule_side = selfplay_considered(c, 0) || selfplay_considered(c, 1);
    const bool rule_unguarded = c.run == kRunSolve && rule_side && !guarded && !t.outcome && !t.proven;
    // gbl_collect_gumbel_tb likewise: a call with a Gumbel side that reads the table runs its own kernel; one that does not read it (no
    // TABLEBASE side, no judge array) is gbl_collect_search_gumbel's launch, and one without a Gumbel side gbl_collect_search_tb's below
    // (depths and weights 0) -- with no EVAL_TREE side at all its search-free instantiation
    const bool rule_table = c.run == kRunTb && rule_side && reads_table;
    const bool rule_untabled = c.run == kRunTb && rule_side && !reads_table;
    // (a call that never reads the table passes an empty one: no ply probes)
    const TbPlay tb{static_cast<const uint8_t *>(c.aux), c.table, reads_table ? tb_shape(c.inventory) : TbShape{}, c.tb_mode, c.tb_count,
                    (t.tb_outcome || t.tb_value || t.tb_played) ? 1 : 0, t.tb_outcome, t.tb_value, t.tb_played};
    if (uct) {
        // the larger leaf of the sides that search
        const int wide = std::max(1, std::max(c.policy[0] == GBL_POLICY_TREE ? c.playouts[0] : 0, c.policy[1] == GBL_POLICY_TREE ? c.playouts[1] : 0));
#define GBL_CS(W)                                                                                                                         \
    hipLaunchKernelGGL((k_collect_search<W>), grid, dim3(64 * W), lds, s, c.state, c.to_move, c.n, c.seed, c.env_base, c.ply_dev, c.ply0,    \
                       c.plies, c.done, c.ply_stride, c.tile_stride, T, c.policy[0], c.policy[1], its0, its1, (uint32_t)c.playouts[0],       \
                       (uint32_t)c.playouts[1], (uint32_t)c.max_plies, explore, c.sample_plies, c.illegal_mode, c.counters, c.turn)
        switch (tree_waves(c.n, wide)) {
        case 4: GBL_CS(4); break;
        case 2: GBL_CS(2); break;
        default: GBL_CS(1); break;
        }
#undef GBL_CS
        GBL_LAUNCHED(name);
    }
    // the evaluator family: one argument struct for the kernels that take it (a side that does not search has weight 0, share 256, considered 0)
    const uint32_t w0 = c.policy[0] == GBL_POLICY_EVAL_TREE ? (uint32_t)c.noise[0] : 0u,
                   w1 = c.policy[1] == GBL_POLICY_EVAL_TREE ? (uint32_t)c.noise[1] : 0u;
    const uint32_t sh0 = (uint32_t)selfplay_share(c, 0), sh1 = (uint32_t)selfplay_share(c, 1);
    const uint32_t m0 = (uint32_t)selfplay_considered(c, 0), m1 = (uint32_t)selfplay_considered(c, 1);
    const SelfplayArgs a{c.ply_stride, c.tile_stride, T, t.root_value, t.priors, t.outcome, t.proven, nets[0], nets[1], c.policy[0], c.policy[1],
                         its0, its1, c.solve_depth[0], c.solve_depth[1], w0, w1, m0, m1, (uint32_t)most, explore, c.sample_plies, c.illegal_mode, c.counters, c.turn,
                         GumbelArgs{0u, (uint32_t)c.gumbel_noise, (uint32_t)c.visit_offset, (uint32_t)c.scale}, tb};
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(64), lds, s, c.state, c.to_move, c.n, c.seed, c.env_base, c.ply_dev, c.ply0, c.plies, c.done, a);
    };
#define GBL_CSV(NOISE, CAP)                                                                                                               \
    hipLaunchKernelGGL((k_collect_solve<NOISE, CAP>), grid, dim3(64), lds, s, c.state, c.to_move, c.n, c.seed, c.env_base, c.ply_dev, c.ply0, \
                       c.plies, c.done, c.ply_stride, c.tile_stride, T, t.root_value, t.priors, t.outcome, t.proven, nets[0], nets[1],       \
                       c.policy[0], c.policy[1], its0, its1, c.solve_depth[0], c.solve_depth[1], (uint32_t)most, explore, c.sample_plies,    \
                       c.illegal_mode, c.counters, c.turn, w0, w1, (uint32_t)c.fast[0], (uint32_t)c.fast[1], sh0, sh1)
    const bool cap = sh0 < (uint32_t)kCapFullShare || sh1 < (uint32_t)kCapFullShare;
    if (rule_table)
        launch(k_collect_gumbel_tb);
    else if (c.run == kRunSolve && rule_side && !rule_unguarded)
        hipLaunchKernelGGL(k_collect_gumbel_solve, grid, dim3(64), lds, s, c.state, c.to_move, c.n, c.seed, c.env_base, c.ply_dev, c.ply0, c.plies,
                           c.done, c.ply_stride, c.tile_stride, T, t.root_value, t.priors, t.outcome, t.proven, nets[0], nets[1], c.policy[0],
                           c.policy[1], its0, its1, c.solve_depth[0], c.solve_depth[1], (uint32_t)most, explore, c.sample_plies, c.illegal_mode,
                           c.counters, c.turn, a.gum, m0, m1);
    else if (c.run == kRunEval || rule_unguarded || rule_untabled)
        // (k_collect_eval<false> is the kernel without the rule's code: gbl_collect_search_eval, and gbl_collect_search_gumbel with no Gumbel side)
        (m0 | m1) ? launch(k_collect_eval<true>) : launch(k_collect_eval<false>);
    else if (c.run == kRunTb && most == 0)  // (no side searches: the instantiation without the solver and the tree)
        launch(k_collect_tb<false, false>);
    else if (c.run == kRunTb)
        (w0 | w1) ? launch(k_collect_tb<true, true>) : launch(k_collect_tb<false, true>);
    // (k_collect_solve<false, ...> is the kernel without the noise's code: both weights 0 run it, whichever entry point asked; and
    // <..., false> the one without the cap's: both shares 256 run it)
    else if (cap && (w0 | w1))
        GBL_CSV(true, true);
    else if (cap)
        GBL_CSV(false, true);
    else if (w0 | w1)
        GBL_CSV(true, false);
    else
        GBL_CSV(false, false);
#undef GBL_CSV
    GBL_LAUNCHED(name);
}

// the nine entry points themselves: one text for both flavours
#define GBL_SYMBOL(fn) gbl_##fn
#define GBL_SELFPLAY_RUN(name, call, stream) selfplay_launch(name, call, stream)
#include "gobblet_selfplay_entries.inc"
#include "gobblet_env_entries.inc"  // (gbl_step, _step_into, _sample, _rollout, _collect, _collect_from, _greedy_act: they only forward)
#undef GBL_SYMBOL
#undef GBL_SELFPLAY_RUN

int gbl_outcome_targets(const int8_t *done_traj, const int8_t *reward_traj, const int8_t *mover_traj, int8_t *z_traj,
                        int16_t *plies_left_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint32_t plies, void *stream)
{
    if (const char *why = outcome_targets_error(n, done_traj, reward_traj, mover_traj, z_traj, plies, ply_stride, tile_stride))
        return fail(GBL_ERR_ARG, why);
    if (n == 0 || plies == 0) return GBL_OK;
    if (off(2, reward_traj)) return fail(GBL_ERR_ALIGN, "reward_traj must be 2-byte aligned");
    if (off(2, plies_left_traj)) return fail(GBL_ERR_ALIGN, "plies_left_traj must be 2-byte aligned");
    const int64_t ntiles = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_outcome_targets, dim3((uint32_t)std::min<int64_t>(ntiles, 1 << 20)), dim3(64), 0, (hipStream_t)stream, done_traj,
                       reward_traj, mover_traj, z_traj, plies_left_traj, n, ntiles, ply_stride, tile_stride, plies);
    GBL_LAUNCHED("gbl_outcome_targets");
}

int gbl_symmetry_apply(const int16_t *sym, int sym_all, const int8_t *agent, const int8_t *state_in, int8_t *state_out,
                       const int8_t *obs_in, int8_t *obs_out, const int8_t *mask_in, int8_t *mask_out, const int16_t *visits_in,
                       int16_t *visits_out, const uint8_t *priors_in, uint8_t *priors_out, const int32_t *actions_in,
                       int32_t *actions_out, int64_t n, void *stream)
{
    const SymRowsArg Q{{state_in, obs_in, mask_in, visits_in, priors_in, actions_in},
                       {state_out, obs_out, mask_out, visits_out, priors_out, actions_out}};
    if (const char *why = symmetry_error(sym, sym_all, agent, Q, n)) return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(state_in, "state_in"); GBL_ALIGNED(state_out, "state_out"); GBL_ALIGNED(obs_in, "obs_in"); GBL_ALIGNED(obs_out, "obs_out");
    GBL_ALIGNED(mask_in, "mask_in"); GBL_ALIGNED(mask_out, "mask_out"); GBL_ALIGNED(visits_in, "visits_in");
    GBL_ALIGNED(visits_out, "visits_out"); GBL_ALIGNED(priors_in, "priors_in"); GBL_ALIGNED(priors_out, "priors_out");
    if (off(4, actions_in, actions_out)) return fail(GBL_ERR_ALIGN, "actions_in / actions_out must be 4-byte aligned");
    if (off(2, sym)) return fail(GBL_ERR_ALIGN, "sym must be 2-byte aligned");
    const Geometry g = geometry(n);
    const SymRows R{state_in,  obs_in,  mask_in,  visits_in,  priors_in, actions_in,
                    state_out, obs_out, mask_out, visits_out, priors_out, actions_out};
    hipLaunchKernelGGL(k_symmetry_apply, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, sym, sym_all, agent, R, n, g.ntiles);
    GBL_LAUNCHED("gbl_symmetry_apply");
}

int gbl_training_batch(const int8_t *obs_traj, const int8_t *mask_traj, const int16_t *visits_traj, const int8_t *z_traj,
                       const int8_t *done_traj, const int8_t *mover_traj, int64_t n, uint32_t plies, int64_t ply_stride,
                       int64_t tile_stride, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base, uint32_t call,
                       int8_t *obs_out, int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out, int16_t *sym_out,
                       void *stream)
{
    if (const char *why = batch_error(obs_traj, mask_traj, visits_traj, z_traj, done_traj, mover_traj, n, plies, ply_stride, tile_stride,
                                      batch, sym_mask, call, obs_out, mask_out, index_out))
        return fail(GBL_ERR_ARG, why);
    if (batch == 0) return GBL_OK;
    GBL_ALIGNED(obs_out, "obs_out"); GBL_ALIGNED(mask_out, "mask_out"); GBL_ALIGNED(visits_out, "visits_out");
    if (off(4, visits_traj, index_out)) return fail(GBL_ERR_ALIGN, "visits_traj / index_out must be 4-byte aligned");
    if (off(2, sym_out)) return fail(GBL_ERR_ALIGN, "sym_out must be 2-byte aligned");
    const Geometry g = geometry(batch);
    const BatchArgs A{obs_traj, mask_traj, visits_traj, z_traj, done_traj, mover_traj, obs_out, mask_out, visits_out, z_out, index_out, sym_out,
                      n, ply_stride, tile_stride, batch, g.ntiles, seed, sample_base, plies, call, (uint32_t)sym_mask};
    hipLaunchKernelGGL(k_training_batch, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, A);
    GBL_LAUNCHED("gbl_training_batch");
}

size_t gbl_replay_workspace_bytes(int64_t n, uint32_t plies) { return (size_t)replay_workspace_bytes(n, plies); }

int gbl_replay_append(const int8_t *obs_traj, const int8_t *mask_traj, const int16_t *visits_traj, const int8_t *z_traj,
                      const int8_t *done_traj, const int8_t *mover_traj, int64_t n, uint32_t plies, int64_t ply_stride,
                      int64_t tile_stride, int32_t tag, int8_t *ring_obs, int16_t *ring_visits, int8_t *ring_meta, int64_t capacity,
                      uint64_t *ring_state, void *workspace, size_t workspace_bytes, void *stream)
{
    if (const char *why = replay_append_error(obs_traj, mask_traj, visits_traj, z_traj, done_traj, mover_traj, n, plies, ply_stride,
                                              tile_stride, ring_obs, ring_visits, ring_meta, capacity, ring_state, workspace, workspace_bytes))
        return fail(GBL_ERR_ARG, why);
    if (off(128, ring_obs, ring_visits, ring_meta)) return fail(GBL_ERR_ALIGN, "ring_obs / ring_visits / ring_meta must be 128-byte aligned");
    GBL_ALIGNED(ring_state, "ring_state"); GBL_ALIGNED(workspace, "workspace");
    GBL_ALIGNED(obs_traj, "obs_traj"); GBL_ALIGNED(mask_traj, "mask_traj"); GBL_ALIGNED(visits_traj, "visits_traj");
    const int64_t ntiles = (n + kTile - 1) / kTile, chunks = replay_chunks(n, plies);
    const ReplayAppendArgs A{obs_traj, mask_traj, visits_traj, z_traj, done_traj, mover_traj, ring_obs, ring_visits, ring_meta, ring_state,
                             static_cast<uint64_t *>(workspace), n, ply_stride, tile_stride, ntiles, chunks, (uint64_t)capacity, tag};
    const dim3 grid((uint32_t)std::min<int64_t>(chunks, kReplayMaxGrid));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_replay_count, grid, dim3(64), 0, s, A);
    GBL_LAUNCH_CHECK("gbl_replay_append");
    hipLaunchKernelGGL(k_replay_scan, dim3(1), dim3(kReplayScanThreads), 0, s, A);
    GBL_LAUNCH_CHECK("gbl_replay_append");
    hipLaunchKernelGGL(k_replay_scatter, grid, dim3(64), 0, s, A);
    GBL_LAUNCHED("gbl_replay_append");
}

int gbl_replay_batch(const int8_t *ring_obs, const int16_t *ring_visits, const int8_t *ring_meta, int64_t capacity,
                     const uint64_t *ring_state, int64_t recent, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base,
                     uint32_t call, int8_t *obs_out, int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out,
                     int16_t *sym_out, void *stream)
{
    if (const char *why = replay_batch_error(ring_obs, ring_visits, ring_meta, capacity, ring_state, recent, batch, sym_mask, call, obs_out,
                                             index_out))
        return fail(GBL_ERR_ARG, why);
    if (batch == 0) return GBL_OK;
    if (off(128, ring_obs, ring_visits, ring_meta)) return fail(GBL_ERR_ALIGN, "ring_obs / ring_visits / ring_meta must be 128-byte aligned");
    GBL_ALIGNED(ring_state, "ring_state");
    GBL_ALIGNED(obs_out, "obs_out"); GBL_ALIGNED(mask_out, "mask_out"); GBL_ALIGNED(visits_out, "visits_out");
    if (off(4, index_out)) return fail(GBL_ERR_ALIGN, "index_out must be 4-byte aligned");
    if (off(2, sym_out)) return fail(GBL_ERR_ALIGN, "sym_out must be 2-byte aligned");
    const Geometry g = geometry(batch);
    const ReplayBatchArgs A{ring_obs, ring_visits, ring_meta, ring_state, obs_out, mask_out, visits_out, z_out, index_out, sym_out,
                            batch, g.ntiles, recent, (uint64_t)capacity, seed, sample_base, call, (uint32_t)sym_mask};
    hipLaunchKernelGGL(k_replay_batch, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, A);
    GBL_LAUNCHED("gbl_replay_batch");
}

size_t gbl_replay_prio_index_bytes(int64_t capacity) { return (size_t)replay_prio_index_bytes(capacity); }

int gbl_replay_prio_append(const int16_t *visits_traj, const int8_t *z_traj, const int8_t *done_traj, const int32_t *prio_traj, int32_t value,
                           int64_t n, uint32_t plies, int64_t ply_stride, int64_t tile_stride, int32_t *ring_prio, int64_t capacity,
                           const uint64_t *ring_state, const void *workspace, size_t workspace_bytes, void *stream)
{
    if (const char *why = replay_prio_append_error(visits_traj, z_traj, done_traj, n, plies, ply_stride, tile_stride, ring_prio, capacity,
                                                   ring_state, workspace, workspace_bytes))
        return fail(GBL_ERR_ARG, why);
    if (off(128, ring_prio)) return fail(GBL_ERR_ALIGN, "ring_prio must be 128-byte aligned");
    GBL_ALIGNED(ring_state, "ring_state"); GBL_ALIGNED(workspace, "workspace");
    if (off(4, prio_traj)) return fail(GBL_ERR_ALIGN, "prio_traj must be 4-byte aligned");
    const int64_t ntiles = (n + kTile - 1) / kTile, chunks = replay_chunks(n, plies);
    const ReplayPrioAppendArgs A{prio_traj, ring_prio, static_cast<const uint64_t *>(workspace), ply_stride, tile_stride, ntiles, chunks,
                                 (uint64_t)capacity, value};
    hipLaunchKernelGGL(k_replay_prio_append, dim3((uint32_t)std::min<int64_t>(chunks, kReplayMaxGrid)), dim3(64), 0, (hipStream_t)stream, A);
    GBL_LAUNCHED("gbl_replay_prio_append");
}

int gbl_replay_prio_update(const int32_t *index, const int32_t *values, int64_t batch, int32_t *ring_prio, int64_t capacity, void *stream)
{
    if (const char *why = replay_prio_update_error(index, values, batch, ring_prio, capacity)) return fail(GBL_ERR_ARG, why);
    if (batch == 0) return GBL_OK;
    if (off(128, ring_prio)) return fail(GBL_ERR_ALIGN, "ring_prio must be 128-byte aligned");
    if (off(4, index, values)) return fail(GBL_ERR_ALIGN, "index / values must be 4-byte aligned");
    const dim3 grid((uint32_t)std::min<int64_t>((batch + 255) / 256, kReplayMaxGrid));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_replay_prio_update<0>, grid, dim3(256), 0, s, index, values, batch, ring_prio, capacity);
    GBL_LAUNCH_CHECK("gbl_replay_prio_update");
    hipLaunchKernelGGL(k_replay_prio_update<1>, grid, dim3(256), 0, s, index, values, batch, ring_prio, capacity);
    GBL_LAUNCHED("gbl_replay_prio_update");
}

int gbl_replay_prio_index(const int32_t *ring_prio, int64_t capacity, const uint64_t *ring_state, void *prio_index, size_t index_bytes,
                          void *stream)
{
    if (const char *why = replay_prio_index_error(ring_prio, capacity, ring_state, prio_index, index_bytes)) return fail(GBL_ERR_ARG, why);
    if (off(128, ring_prio)) return fail(GBL_ERR_ALIGN, "ring_prio must be 128-byte aligned");
    GBL_ALIGNED(ring_state, "ring_state"); GBL_ALIGNED(prio_index, "prio_index");
    const uint64_t leaves = replay_prio_leaves((uint64_t)capacity), blocks = replay_prio_blocks((uint64_t)capacity);
    const ReplayPrioIndexArgs A{ring_prio, ring_state, static_cast<uint64_t *>(prio_index), (uint64_t)capacity, leaves, blocks};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_replay_prio_leaves, dim3((uint32_t)std::min<uint64_t>(blocks, 1u << 16)), dim3(kReplayLeafThreads), 0, s, A);
    GBL_LAUNCH_CHECK("gbl_replay_prio_index");
    hipLaunchKernelGGL(k_replay_prio_scan, dim3(1), dim3(kReplayScanThreads), 0, s, A);
    GBL_LAUNCHED("gbl_replay_prio_index");
}

int gbl_replay_batch_prio(const int8_t *ring_obs, const int16_t *ring_visits, const int8_t *ring_meta, int64_t capacity,
                          const uint64_t *ring_state, const int32_t *ring_prio, const void *prio_index, int32_t *prio_out, uint64_t *total_out,
                          int64_t recent, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base, uint32_t call, int8_t *obs_out,
                          int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out, int16_t *sym_out, void *stream)
{
    if (const char *why = replay_batch_prio_error(ring_obs, ring_visits, ring_meta, capacity, ring_state, ring_prio, prio_index, recent, batch,
                                                  sym_mask, call, obs_out, index_out))
        return fail(GBL_ERR_ARG, why);
    if (batch == 0) return GBL_OK;
    if (off(128, ring_obs, ring_visits, ring_meta)) return fail(GBL_ERR_ALIGN, "ring_obs / ring_visits / ring_meta must be 128-byte aligned");
    if (off(128, ring_prio)) return fail(GBL_ERR_ALIGN, "ring_prio must be 128-byte aligned");
    GBL_ALIGNED(ring_state, "ring_state"); GBL_ALIGNED(prio_index, "prio_index");
    GBL_ALIGNED(obs_out, "obs_out"); GBL_ALIGNED(mask_out, "mask_out"); GBL_ALIGNED(visits_out, "visits_out");
    if (off(4, index_out, prio_out)) return fail(GBL_ERR_ALIGN, "index_out / prio_out must be 4-byte aligned");
    if (off(8, total_out)) return fail(GBL_ERR_ALIGN, "total_out must be 8-byte aligned");
    if (off(2, sym_out)) return fail(GBL_ERR_ALIGN, "sym_out must be 2-byte aligned");
    const Geometry g = geometry(batch);
    const ReplayBatchPrioArgs A{{ring_obs, ring_visits, ring_meta, ring_state, obs_out, mask_out, visits_out, z_out, index_out, sym_out,
                                 batch, g.ntiles, recent, (uint64_t)capacity, seed, sample_base, call, (uint32_t)sym_mask},
                                ring_prio, static_cast<const uint64_t *>(prio_index), prio_out, total_out};
    hipLaunchKernelGGL(k_replay_batch_prio, dim3(g.grid), dim3(64), 0, (hipStream_t)stream, A);
    GBL_LAUNCHED("gbl_replay_batch_prio");
}

int gbl_tb_layout(const int32_t *inventory, int64_t *out)
{
    if (const char *why = tb_inventory_error(inventory)) return fail(GBL_ERR_ARG, why);
    GBL_NEED(out, "out");
    const TbShape S = tb_shape(inventory);
    out[0] = (int64_t)S.positions;
    for (int k = 0; k < 3; ++k) out[1 + k] = S.L[k];
    out[4] = kTbAuxBytes;
    return GBL_OK;
}

int gbl_tb_prepare(const int32_t *inventory, void *aux, void *stream)
{
    if (const char *why = tb_inventory_error(inventory)) return fail(GBL_ERR_ARG, why);
    if (!aux) return fail(GBL_ERR_ARG, "aux must not be NULL");
    GBL_ALIGNED(aux, "aux");
    hipLaunchKernelGGL(k_tb_prepare, dim3(1), dim3(kTbThreads), 0, (hipStream_t)stream, static_cast<uint8_t *>(aux));
    GBL_LAUNCHED("gbl_tb_prepare");
}

int gbl_tb_sweep(const int32_t *inventory, const void *aux, const int8_t *table, int8_t *out, int64_t first, int64_t count, int k,
                 uint64_t *decided, void *stream)
{
    if (const char *why = tb_sweep_error(inventory, aux, table, out, first, count, k, decided)) return fail(GBL_ERR_ARG, why);
    if (count == 0) return GBL_OK;
    GBL_ALIGNED(aux, "aux");
    if (off(8, decided)) return fail(GBL_ERR_ALIGN, "decided must be 8-byte aligned");
    const TbSweepArgs A{static_cast<const uint32_t *>(aux), table, out, reinterpret_cast<unsigned long long *>(decided), (uint64_t)first,
                        (uint64_t)count, tb_shape(inventory), k};
    // two workgroups per compute unit hold their tables at once (61.6 KB each of 160 KB): no more workgroups than that on 256 CUs, each striding
    const int64_t groups = std::min<int64_t>((count + kTbThreads - 1) / kTbThreads, kTbSweepGroups);
    hipLaunchKernelGGL(k_tb_sweep, dim3((uint32_t)groups), dim3(kTbThreads), 0, (hipStream_t)stream, A);
    GBL_LAUNCHED("gbl_tb_sweep");
}

int gbl_tb_index(const int32_t *inventory, const void *aux, const int8_t *state, const int8_t *to_move, int64_t *index_out, int64_t n,
                 void *stream)
{
    if (const char *why = tb_rows_error(inventory, aux, n, state, "state must not be NULL", to_move, "to_move must not be NULL", index_out,
                                        "index_out must not be NULL"))
        return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(aux, "aux");
    if (off(8, index_out)) return fail(GBL_ERR_ALIGN, "index_out must be 8-byte aligned");
    const int64_t groups = std::min<int64_t>((n + 255) / 256, (int64_t)1 << 20);
    hipLaunchKernelGGL(k_tb_index, dim3((uint32_t)groups), dim3(256), 0, (hipStream_t)stream, static_cast<const uint8_t *>(aux), state, to_move,
                       index_out, n, tb_shape(inventory));
    GBL_LAUNCHED("gbl_tb_index");
}

int gbl_tb_position(const int32_t *inventory, const void *aux, const int64_t *index, int8_t *state_out, int64_t n, void *stream)
{
    if (const char *why = tb_rows_error(inventory, aux, n, index, "index must not be NULL", state_out, "state_out must not be NULL", state_out, ""))
        return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(aux, "aux");
    if (off(8, index)) return fail(GBL_ERR_ALIGN, "index must be 8-byte aligned");
    const int64_t groups = std::min<int64_t>((n + 255) / 256, (int64_t)1 << 20);
    hipLaunchKernelGGL(k_tb_position, dim3((uint32_t)groups), dim3(256), 0, (hipStream_t)stream, static_cast<const uint8_t *>(aux), index,
                       state_out, n, tb_shape(inventory));
    GBL_LAUNCHED("gbl_tb_position");
}

int gbl_tb_probe(const int32_t *inventory, const void *aux, const int8_t *table, const int8_t *state, const int8_t *to_move,
                 const int8_t *mask, int8_t *outcome_out, int8_t *value_out, int32_t *action_out, int64_t n, void *stream)
{
    if (const char *why = tb_rows_error(inventory, aux, n, table, "table must not be NULL", state, "state must not be NULL", to_move,
                                        "to_move must not be NULL"))
        return fail(GBL_ERR_ARG, why);
    if (n == 0) return GBL_OK;
    GBL_ALIGNED(aux, "aux");
    if (off(4, action_out)) return fail(GBL_ERR_ALIGN, "action_out must be 4-byte aligned");
    const int64_t groups = std::min<int64_t>(n, (int64_t)1 << 20);
    hipLaunchKernelGGL(k_tb_probe, dim3((uint32_t)groups), dim3(64), 0, (hipStream_t)stream, static_cast<const uint8_t *>(aux), table, state, to_move,
                       mask, outcome_out, value_out, action_out, n, tb_shape(inventory));
    GBL_LAUNCHED("gbl_tb_probe");
}

int gbl_tb_targets(const int32_t *inventory, const void *aux, const int8_t *table, const int8_t *obs, int64_t obs_pitch, const int8_t *mask,
                   int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch, const int8_t *z_in, int8_t *z_out,
                   int64_t z_pitch, int mode, int count, int8_t *value_out, int8_t *outcome_out, int8_t *census_out, int64_t n, void *stream)
{
    bool empty;
    if (const char *why = tb_targets_error(inventory, aux, table, obs, obs_pitch, mask, mask_pitch, visits_in, visits_out, visits_pitch, z_in,
                                           z_out, z_pitch, mode, count, value_out, outcome_out, census_out, n, &empty))
        return fail(GBL_ERR_ARG, why);
    if (empty) return GBL_OK;
    GBL_ALIGNED(aux, "aux");
    if (off(2, visits_in)) return fail(GBL_ERR_ALIGN, "visits_in must be 2-byte aligned");
    if (off(2, visits_out)) return fail(GBL_ERR_ALIGN, "visits_out must be 2-byte aligned");
    const TbTargetArgs A{static_cast<const uint8_t *>(aux), table, obs, mask, visits_in, visits_out, z_in, z_out, value_out, outcome_out,
                         census_out, obs_pitch, mask_pitch, visits_pitch, z_pitch, n, tb_shape(inventory), mode, count};
    const int64_t groups = std::min<int64_t>((n + kTbTargetWaves - 1) / kTbTargetWaves, kTbTargetGroups);
    hipLaunchKernelGGL(k_tb_targets, dim3((uint32_t)groups), dim3(64 * kTbTargetWaves), 0, (hipStream_t)stream, A);
    GBL_LAUNCHED("gbl_tb_targets");
}

}  // extern "C"

// what gbl_reanalyse and gbl_reanalyse_gumbel do once their arguments have passed reanalyse_error: the network, the alignments, the launch
template <bool GUMBEL, typename Args>
static int reanalyse_launch(const gbl_evaluator *ev, Args A, void *stream, const char *what)
{
    if (const int e = eval_net_of(ev, A.net)) return e;
    if (off(2, A.visits_in)) return fail(GBL_ERR_ALIGN, "visits_in must be 2-byte aligned");
    if (off(2, A.visits_out)) return fail(GBL_ERR_ALIGN, "visits_out must be 2-byte aligned");
    if (off(4, A.root_value_out, A.action_out, A.nodes_out, A.drift_out))
        return fail(GBL_ERR_ALIGN, "root_value_out / action_out / nodes_out / drift_out must be 4-byte aligned");
    if constexpr (GUMBEL)
        if (off(2, A.gumbel_out)) return fail(GBL_ERR_ALIGN, "gumbel_out must be 2-byte aligned");
    // the tree as gbl_tree_search_eval's: a node and a prior row per iteration, and the root's (the rule keeps no LDS)
    const size_t lds = (sizeof(TreeNode) + kEvalOutputs) * ((size_t)A.iterations + 1);
    const int64_t groups = std::min<int64_t>(A.n, knob::kReanalyseGroups);
    hipLaunchKernelGGL(k_reanalyse<GUMBEL>, dim3((uint32_t)groups), dim3(64), lds, (hipStream_t)stream, A);
    GBL_LAUNCHED(what);
}

// gbl_train_step (EX = false: the weighted step's six arguments are not read) and gbl_train_step_weighted under their own names: the
// checks, the kernels' arguments, the launch shape, the rows kernel of hidden / 64 units and the reduction
template <bool EX>
static int train_launch(const char *name, const int8_t *obs, const int8_t *mask, const int16_t *visits, const int8_t *z, int64_t batch, int hidden,
                        float *params, float *adam_m, float *adam_v, const gbl_train_hyper *hyper, const float *row_weight, float *row_loss_out,
                        int32_t *prio_out, float prio_scale, int32_t prio_floor, int32_t prio_cap, float *grad_out, float *stats_out,
                        void *workspace, int64_t workspace_bytes, void *stream)
{
    if (const char *why = train_error(obs, visits, z, batch, hidden, params, adam_m, adam_v, hyper, stats_out, workspace, workspace_bytes))
        return fail(GBL_ERR_ARG, why);
    GBL_ALIGNED(obs, "obs"); GBL_ALIGNED(mask, "mask"); GBL_ALIGNED(visits, "visits"); GBL_ALIGNED(params, "params");
    GBL_ALIGNED(adam_m, "adam_m"); GBL_ALIGNED(adam_v, "adam_v"); GBL_ALIGNED(grad_out, "grad_out"); GBL_ALIGNED(stats_out, "stats_out");
    GBL_ALIGNED(workspace, "workspace");
    if constexpr (EX) {
        if (const char *why = train_weighted_error(prio_out, prio_scale, prio_floor, prio_cap)) return fail(GBL_ERR_ARG, why);
        if (off(4, row_weight, row_loss_out, prio_out)) return fail(GBL_ERR_ALIGN, "row_weight / row_loss_out / prio_out must be 4-byte aligned");
    }
    float *ws = static_cast<float *>(workspace);
    const TrainExArgs X{{obs, mask, visits, z, params, adam_m, adam_v, grad_out, stats_out,
                         ws, ws + batch * hidden, ws + 2 * batch * hidden, ws + 2 * batch * hidden + batch * kTrainDoStride, batch, hidden,
                         TrainHyper{hyper->lr, hyper->beta1, hyper->beta2, hyper->eps, hyper->weight_decay, hyper->value_reg, hyper->bias1,
                                    hyper->bias2}},
                        row_weight, row_loss_out, prio_out, prio_scale, prio_floor, prio_cap};
    const std::conditional_t<EX, TrainExArgs, TrainArgs> &A = X;  // (the rows kernel's own argument type)
    // as many workgroups as stay resident on 256 CUs, at most one per four rows: 4 / 4 / 3 / 2 per CU at H = 64 / 128 / 192 / 256, the
    // smaller of what the registers allow (127 / 127 / 168 / 212 VGPRs: 4 / 4 / 3 / 2 wavefronts per SIMD, a workgroup being one wavefront on
    // each SIMD) and what the LDS allows (w2 and four rows' scratch: 18 / 33 / 48 / 63 KB of 160); the weighted instantiations' registers
    // allow 4 / 4 / 2 / 2
    const int units = hidden / 64;
    const int64_t resident = 256 * (int64_t)(units <= 2 ? 4 : units == 3 && !EX ? 3 : 2);
    const dim3 rows_grid((uint32_t)std::min<int64_t>((batch + kTrainRowWaves - 1) / kTrainRowWaves, resident)), rows_block(64 * kTrainRowWaves);
    const size_t lds = train_rows_lds(hidden);
    hipStream_t s = (hipStream_t)stream;
    if (units == 1) hipLaunchKernelGGL((k_train_rows<1, EX>), rows_grid, rows_block, lds, s, A);
    else if (units == 2) hipLaunchKernelGGL((k_train_rows<2, EX>), rows_grid, rows_block, lds, s, A);
    else if (units == 3) hipLaunchKernelGGL((k_train_rows<3, EX>), rows_grid, rows_block, lds, s, A);
    else hipLaunchKernelGGL((k_train_rows<4, EX>), rows_grid, rows_block, lds, s, A);
    GBL_LAUNCH_CHECK(name);
    const uint32_t tiles = (uint32_t)((train_param_count(hidden) + 3 + 63) / 64);  // (+ 3: the statistics' lanes)
    hipLaunchKernelGGL(k_train_reduce_adam, dim3(tiles), dim3(64 * kTrainReduceWaves), 0, s, static_cast<const TrainArgs &>(X));
    GBL_LAUNCHED(name);
}

extern "C" {

int gbl_reanalyse(const gbl_evaluator *ev, int iterations, int explore, const int8_t *obs, int64_t obs_pitch, const int8_t *mask,
                  int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch, const int8_t *z_in, int64_t z_pitch,
                  int32_t *root_value_out, uint8_t *root_priors_out, int32_t *action_out, int32_t *nodes_out, int32_t *drift_out,
                  int8_t *census_out, int64_t n, void *stream)
{
    bool empty;
    if (const char *why = reanalyse_error(ev, iterations, explore, obs, obs_pitch, mask, mask_pitch, visits_in, visits_out, visits_pitch, z_in,
                                          z_pitch, root_value_out, root_priors_out, action_out, nodes_out, drift_out, census_out, n, &empty))
        return fail(GBL_ERR_ARG, why);
    if (empty) return GBL_OK;
    return reanalyse_launch<false>(ev, ReanalyseArgs{EvalNet{}, obs, mask, visits_in, visits_out, z_in, root_value_out, root_priors_out, action_out,
                                                     nodes_out, drift_out, census_out, obs_pitch, mask_pitch, visits_pitch, z_pitch, n,
                                                     (uint32_t)iterations, (uint32_t)explore},
                                   stream, "gbl_reanalyse");
}

int gbl_reanalyse_gumbel(const gbl_evaluator *ev, int iterations, int explore, int considered, int gumbel_noise, int visit_offset, int scale,
                         uint64_t seed, uint64_t env_base, uint32_t call, const int8_t *obs, int64_t obs_pitch, const int8_t *mask,
                         int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch, const int8_t *z_in,
                         int64_t z_pitch, int32_t *root_value_out, uint8_t *root_priors_out, int32_t *action_out, int32_t *nodes_out,
                         int32_t *drift_out, int8_t *census_out, int16_t *gumbel_out, int64_t n, void *stream)
{
    bool empty;
    const ReanalyseGumbelCheck check{considered, gumbel_noise, visit_offset, scale, env_base, call, gumbel_out};
    if (const char *why = reanalyse_error(ev, iterations, explore, obs, obs_pitch, mask, mask_pitch, visits_in, visits_out, visits_pitch, z_in,
                                          z_pitch, root_value_out, root_priors_out, action_out, nodes_out, drift_out, census_out, n, &empty,
                                          &check))
        return fail(GBL_ERR_ARG, why);
    if (empty) return GBL_OK;
    return reanalyse_launch<true>(
        ev, ReanalyseGumbelArgs{{EvalNet{}, obs, mask, visits_in, visits_out, z_in, root_value_out, root_priors_out, action_out, nodes_out,
                                 drift_out, census_out, obs_pitch, mask_pitch, visits_pitch, z_pitch, n, (uint32_t)iterations, (uint32_t)explore},
                                GumbelArgs{(uint32_t)considered, (uint32_t)gumbel_noise, (uint32_t)visit_offset, (uint32_t)scale},
                                seed, env_base, call, gumbel_out},
        stream, "gbl_reanalyse_gumbel");
}

int64_t gbl_train_workspace_bytes(int64_t batch, int hidden) { return train_workspace_bytes(batch, hidden); }

int gbl_train_step(const int8_t *obs, const int8_t *mask, const int16_t *visits, const int8_t *z, int64_t batch, int hidden,
                   float *params, float *adam_m, float *adam_v, const gbl_train_hyper *hyper, float *grad_out, float *stats_out,
                   void *workspace, int64_t workspace_bytes, void *stream)
{
    return train_launch<false>("gbl_train_step", obs, mask, visits, z, batch, hidden, params, adam_m, adam_v, hyper, nullptr, nullptr, nullptr, 0.f,
                               0, 0, grad_out, stats_out, workspace, workspace_bytes, stream);
}

int gbl_train_step_weighted(const int8_t *obs, const int8_t *mask, const int16_t *visits, const int8_t *z, int64_t batch, int hidden,
                            float *params, float *adam_m, float *adam_v, const gbl_train_hyper *hyper, const float *row_weight,
                            float *row_loss_out, int32_t *prio_out, float prio_scale, int32_t prio_floor, int32_t prio_cap, float *grad_out,
                            float *stats_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    return train_launch<true>("gbl_train_step_weighted", obs, mask, visits, z, batch, hidden, params, adam_m, adam_v, hyper, row_weight,
                              row_loss_out, prio_out, prio_scale, prio_floor, prio_cap, grad_out, stats_out, workspace, workspace_bytes, stream);
}

int gbl_replay_importance(const int32_t *prio, int64_t batch, float beta, float *weights_out, void *stream)
{
    if (const char *why = replay_importance_error(prio, batch, beta, weights_out)) return fail(GBL_ERR_ARG, why);
    if (off(4, prio, weights_out)) return fail(GBL_ERR_ALIGN, "prio / weights_out must be 4-byte aligned");
    // (the kernel's loops stride by the grid: one workgroup that walks the batch twice is the same kernel on a grid of 1, the experiment
    // builds' other form -- measured slower from batch 1 024 on: DESIGN.md 5.24)
    const dim3 grid(knob::kImportanceOneGroup ? 1u : (uint32_t)((batch + kImportanceThreads - 1) / kImportanceThreads));
    hipLaunchKernelGGL(k_replay_importance, grid, dim3(kImportanceThreads), 0, (hipStream_t)stream, prio, batch, beta, weights_out);
    GBL_LAUNCHED("gbl_replay_importance");
}

}  // extern "C"

GBL_KNOB_EXTRA_ENTRY_POINTS  // (nothing in the product; an experiment build's run-time form switch: gobblet_ab.h)
