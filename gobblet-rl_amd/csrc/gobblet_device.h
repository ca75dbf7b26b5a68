// gobblet_device.h -- device-side building blocks of the gfx950 Gobblet kernels.
//
// Execution shape: ONE wavefront (64 lanes) per workgroup, ONE board per lane,
// a TILE of 64 consecutive boards per wavefront.  Rows of a tile are contiguous
// in HBM (env-major int8 rows of 27 / 54 / 117 bytes), so a tile is moved with
// full-width 16-byte-per-lane loads/stores (1 KiB per wave instruction) and
// (un)packed to one-row-per-lane through LDS:
//
//   HBM tile --dwordx4--> LDS image --ds_read_b32 + v_alignbyte--> row in VGPRs
//   row in VGPRs --v_alignbyte + ds_write_b32--> LDS image --dwordx4--> HBM tile
//
// Row sizes are odd (27, 54, 117 bytes) so lane l's row starts at byte l*ROWB,
// which is dword-aligned only every 4th (2nd) lane; the byte shift is done in
// registers with v_alignbyte_b32 so that every LDS access is an aligned dword
// and every HBM access a full 16-byte vector.  The 117-byte observation rows are
// the exception on the way out: they are mostly zeros, so the wave zero-fills
// the image and each lane scatters its <= 21 one-bytes (obs_scatter).
//
// The game logic runs on three 27-bit planes per board (bit c = cell c of
// Board.squares, c = 9*level + pos):  nz (cell occupied), neg (player_2's
// piece), odd (piece number odd = first piece of its size).
#pragma once
#ifndef GBL_HOST_EMU  // tests/emu/ compiles this header for the host with shims for the few builtins used
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "gobblet_knobs.h"  // (kGumbelTable)

namespace gbl {

constexpr int kTile = 64;   // boards per wavefront
constexpr int kCells = 27;  // Board.squares, board.py:33
constexpr int kActions = 54;
constexpr int kObs = 117;   // 3*3*13, gobblet.py:145

__device__ __forceinline__ uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t nbytes)
{
    // ({hi,lo} >> 8*nbytes)[31:0], nbytes in 0..3
    return __builtin_amdgcn_alignbyte(hi, lo, nbytes);
}

// Blocks are dealt round-robin over the 8 XCDs (block b and b+8 share one); give every XCD a
// CONTIGUOUS range of tiles so that the 128-byte lines that straddle two tiles are completed inside
// one L2 instead of being written partially by two.  Speed only; any placement is correct.
// Measured (fused kernel): -2.5 % time at 2^20 boards, where the working set lives in the Infinity
// Cache, but +7 % at 2^22, where eight far-apart write fronts cost more in HBM than the shared
// lines save -- so batches beyond 2^21 boards keep the identity map.
constexpr int64_t kXcdRemapMaxTiles = (int64_t)1 << 15;

__device__ __forceinline__ int64_t xcd_tile(uint32_t bid, int64_t ntiles)
{
    if (ntiles > kXcdRemapMaxTiles) return (int64_t)bid;
    int64_t chunk = (ntiles + 7) >> 3;
    return (int64_t)(bid & 7u) * chunk + (bid >> 3);
}

// ---- tile <-> LDS image ---------------------------------------------------------------
// g points at the tile's first byte (16-byte aligned); rows = valid boards in the tile.
// Full tiles move as 16-byte vectors, lane l handling vectors l, l+64, ... : every wave
// instruction covers 1 KiB of contiguous HBM.  All loads of a tile are issued before the first
// dependent LDS write (and all LDS reads before the first store) so they overlap.
// NT = store policy (kStorePlain / kStoreStream / kStoreStreamDrop, see store16).  It is a TEMPLATE parameter on purpose:
// as a runtime flag the `if (nt) nontemporal-store else store` pair is merged by the optimiser into
// one plain store and the hint is silently lost.
typedef uint32_t __attribute__((ext_vector_type(4))) vec4u;

// Store policies of a tile's 16-byte vectors.  kStoreStream = non-temporal hint (`nt`).  kStoreStreamDrop = `nt sc1`:
// the same, and the line does not stay in the XCD's L2 -- for write-once streams and outputs nothing on the GPU reads
// back (2-4 % over `nt` on the trajectory stream, 0.5-2 % on the one-ply kernels' observation stream, in-process A/B
// scripts/ab_inproc.py; `sc1`, `sc0 sc1`, `sc0` without `nt`: 22 % slower at 2^20 boards).  There is no builtin for that
// combination on a global store; the raw BUFFER store builtin takes the cache-policy bits (gfx940 encoding: nt = 2,
// sc1 = 16), so the tile is addressed through a buffer descriptor of exactly its size.  (An inline-assembly store was
// tried first and is WRONG: the compiler does not know it reads its data registers and overwrites them too early.)
constexpr int kStorePlain = 0, kStoreStream = 1, kStoreStreamDrop = 2;

template <int POLICY>
__device__ __forceinline__ void store16(uint4 *dst, const uint4 &v)
{
    static_assert(POLICY == kStorePlain || POLICY == kStoreStream, "kStoreStreamDrop goes through a buffer descriptor (tile_out)");
#ifndef GBL_HOST_EMU
    if (POLICY == kStoreStream) {
        vec4u t = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(t, reinterpret_cast<vec4u *>(dst));
        return;
    }
#endif
    *dst = v;
}

// `between` runs after the tile's global loads have been issued and before the first dependent LDS
// write: work that does not depend on the tile (e.g. the Philox draw) placed there overlaps the
// load latency instead of lengthening the wave's serial path.
#ifndef GBL_HOST_EMU
#define GBL_PIN4(a) "v"((a).x), "v"((a).y), "v"((a).z), "v"((a).w)
template <int N>
__device__ __forceinline__ void pin_loads(const uint4 (&v)[N])
{
    // ONE asm statement per (up to) four vectors: separate statements would let the scheduler slide a
    // later vector's load behind an earlier statement and serialise the round trips again
    if constexpr (N == 1) asm volatile("" ::GBL_PIN4(v[0]) : "memory");
    else if constexpr (N == 2) asm volatile("" ::GBL_PIN4(v[0]), GBL_PIN4(v[1]) : "memory");
    else if constexpr (N == 3) asm volatile("" ::GBL_PIN4(v[0]), GBL_PIN4(v[1]), GBL_PIN4(v[2]) : "memory");
    else {
        asm volatile("" ::GBL_PIN4(v[0]), GBL_PIN4(v[1]), GBL_PIN4(v[2]), GBL_PIN4(v[3]) : "memory");
        if constexpr (N > 4) {
            uint4 rest[N - 4];
#pragma unroll
            for (int i = 0; i < N - 4; ++i) rest[i] = v[i + 4];
            pin_loads<N - 4>(rest);
        }
    }
}
#endif

struct NoWork {
    __device__ __forceinline__ void operator()() const {}
};

template <int ROWB, typename Between = NoWork>
__device__ __forceinline__ void tile_in(const int8_t *__restrict__ g, uint32_t *lds, int lane, int rows,
                                        Between between = Between())
{
    constexpr int NV = kTile * ROWB / 16, FULL = NV / 64, REM = NV % 64;
    if (rows == kTile) {
        const uint4 *gv = reinterpret_cast<const uint4 *>(g);
        uint4 *lv = reinterpret_cast<uint4 *>(lds);
        uint4 v[FULL + 1];
#pragma unroll
        for (int i = 0; i < FULL; ++i) v[i] = gv[lane + 64 * i];
        if (REM) v[FULL] = gv[lane < REM ? lane + 64 * FULL : NV - 1];  // branch-free (a branch would pin the wait)
        between();
#ifndef GBL_HOST_EMU
        // Keep the LDS writes (and their s_waitcnt) behind `between`, and keep EVERY load of the tile up
        // here, issued back to back: naming all loaded dwords as operands stops the optimiser from sinking
        // the last vector's load into the `lane < REM` branch below (or splitting it), and from moving the
        // other loads behind this point -- either would cost a second, serial round trip to memory.
        pin_loads<FULL + 1>(v);
#endif
#pragma unroll
        for (int i = 0; i < FULL; ++i) lv[lane + 64 * i] = v[i];
        if (REM && lane < REM) lv[lane + 64 * FULL] = v[FULL];
    } else {
        // ragged last tile: the whole vectors of its rows in one round trip (clamped to the last whole one: nothing beyond the rows
        // is read), then the last few bytes -- byte by byte all the way it was up to 27 serial round trips per launch (round 5)
        const int bytes = rows * ROWB, nvec = bytes >> 4;
        const uint4 *gv = reinterpret_cast<const uint4 *>(g);
        uint4 *lv = reinterpret_cast<uint4 *>(lds);
        int8_t *lb = reinterpret_cast<int8_t *>(lds);
        uint4 v[FULL + 1];
        const int last = nvec > 0 ? nvec - 1 : 0;
#pragma unroll
        for (int i = 0; i <= FULL; ++i) v[i] = nvec > 0 ? gv[lane + 64 * i < nvec ? lane + 64 * i : last] : uint4{0u, 0u, 0u, 0u};
        const int ti = (nvec << 4) + lane;
        const int8_t tb = ti < bytes ? g[ti] : (int8_t)0;
        between();
#pragma unroll
        for (int i = 0; i <= FULL; ++i)
            if (lane + 64 * i < nvec) lv[lane + 64 * i] = v[i];
        if (ti < bytes) lb[ti] = tb;
    }
}

template <int ROWB, int NT = kStorePlain>
__device__ __forceinline__ void tile_out(int8_t *__restrict__ g, const uint32_t *lds, int lane, int rows)
{
    constexpr int NV = kTile * ROWB / 16, FULL = NV / 64, REM = NV % 64;
    if (rows == kTile) {
        uint4 *gv = reinterpret_cast<uint4 *>(g);
        const uint4 *lv = reinterpret_cast<const uint4 *>(lds);
        // (with cached stores and a 117-byte row the compiler keeps v[] in 144 B of scratch; the
        // observation stream is always stored non-temporally, where it does not -- measured 0.3 %
        // faster than forms that avoid the scratch in the unused variant)
        uint4 v[FULL + 1];
#pragma unroll
        for (int i = 0; i < FULL; ++i) v[i] = lv[lane + 64 * i];
        if (REM && lane < REM) v[FULL] = lv[lane + 64 * FULL];
#ifndef GBL_HOST_EMU
        if constexpr (NT == kStoreStreamDrop) {
            // raw buffer stores with cache policy nt | sc1 (see store16); the descriptor covers exactly this tile
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(g, 0, kTile * ROWB, 0x00020000);
#pragma unroll
            for (int i = 0; i < FULL; ++i) {
                vec4u t = {v[i].x, v[i].y, v[i].z, v[i].w};
                __builtin_amdgcn_raw_buffer_store_b128(t, rs, (lane + 64 * i) * 16, 0, 2 | 16);
            }
            if (REM && lane < REM) {
                vec4u t = {v[FULL].x, v[FULL].y, v[FULL].z, v[FULL].w};
                __builtin_amdgcn_raw_buffer_store_b128(t, rs, (lane + 64 * FULL) * 16, 0, 2 | 16);
            }
            return;
        }
#endif
        constexpr int P = NT == kStoreStreamDrop ? kStoreStream : NT;  // (host emulation: a plain copy either way)
#pragma unroll
        for (int i = 0; i < FULL; ++i) store16<P>(&gv[lane + 64 * i], v[i]);
        if (REM && lane < REM) store16<P>(&gv[lane + 64 * FULL], v[FULL]);
    } else {
        // the ragged last tile: the whole 16-byte vectors of its rows, then the last few bytes (byte by byte all the way it was up
        // to 115 round trips, ~3 us, and a launch lasts as long as its slowest tile: 65 599 boards ran 4.66 us per ply where 65 536
        // run 1.70 -- round 5).  A compact loop, NOT the unrolled fetch-then-store of the whole tiles: unrolled, the compiler
        // re-balanced k_collect around it (111 -> 93 VGPRs) and the 2^20-board launch lost 2 %.
        const int bytes = rows * ROWB, nvec = bytes >> 4;
        uint4 *gv = reinterpret_cast<uint4 *>(g);
        const uint4 *lv = reinterpret_cast<const uint4 *>(lds);
#pragma nounroll
        for (int i = lane; i < nvec; i += 64) gv[i] = lv[i];
        const int8_t *lb = reinterpret_cast<const int8_t *>(lds);
        const int i = (nvec << 4) + lane;
        if (i < bytes) g[i] = lb[i];
    }
}

// tile_out for kernels that are NOT bound by their stores (gbl_collect_policy: the greedy decision dominates): at most
// CHUNK vectors per lane in registers at a time instead of the whole tile (the observation tile alone is 8 vectors = 32
// VGPRs, which there would cost a wavefront of occupancy).  Same bytes, same store policy.
template <int ROWB, int NT, int CHUNK>
__device__ __forceinline__ void tile_out_narrow(int8_t *__restrict__ g, const uint32_t *lds, int lane, int rows)
{
    constexpr int NV = kTile * ROWB / 16;
    if (rows != kTile) {
        tile_out<ROWB, NT>(g, lds, lane, rows);  // (ragged last tile: byte granular)
        return;
    }
    const uint4 *lv = reinterpret_cast<const uint4 *>(lds);
#ifndef GBL_HOST_EMU
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(g, 0, kTile * ROWB, 0x00020000);
#endif
#pragma unroll
    for (int i0 = 0; i0 < NV; i0 += 64 * CHUNK) {
        uint4 v[CHUNK];
#pragma unroll
        for (int u = 0; u < CHUNK; ++u) {
            const int i = i0 + 64 * u + lane;
            v[u] = lv[i < NV ? i : NV - 1];
        }
#pragma unroll
        for (int u = 0; u < CHUNK; ++u) {
            const int i = i0 + 64 * u + lane;
            if (i0 + 64 * u < NV && i < NV) {
#ifndef GBL_HOST_EMU
                if constexpr (NT == kStoreStreamDrop) {
                    vec4u t = {v[u].x, v[u].y, v[u].z, v[u].w};
                    __builtin_amdgcn_raw_buffer_store_b128(t, rs, i * 16, 0, 2 | 16);
                } else
#endif
                    store16<NT == kStoreStreamDrop ? kStoreStream : NT>(reinterpret_cast<uint4 *>(g) + i, v[u]);
            }
        }
    }
}

// tile_out in two halves, for a wavefront that takes a FULL tile's image over from another one: tile_fetch copies
// the image into registers (after which the image may be rebuilt), tile_store sends them out.
template <int ROWB>
__device__ __forceinline__ void tile_fetch(const uint32_t *lds, int lane, uint4 (&v)[kTile * ROWB / 16 / 64 + 1])
{
    constexpr int NV = kTile * ROWB / 16, FULL = NV / 64, REM = NV % 64;
    const uint4 *lv = reinterpret_cast<const uint4 *>(lds);
#pragma unroll
    for (int i = 0; i < FULL; ++i) v[i] = lv[lane + 64 * i];
    v[FULL] = lv[REM && lane < REM ? lane + 64 * FULL : lane];
}

// `bytes`: what of the image leaves -- the whole tile, or the WHOLE vectors of a ragged last tile's rows (a multiple of 16; its
// last few bytes go out with sub_tail while the image still stands)
template <int ROWB, int NT = kStorePlain>
__device__ __forceinline__ void tile_store(int8_t *__restrict__ g, const uint4 (&v)[kTile * ROWB / 16 / 64 + 1], int lane,
                                           int bytes = kTile * ROWB)
{
    constexpr int NV = kTile * ROWB / 16, FULL = NV / 64, REM = NV % 64;
#ifndef GBL_HOST_EMU
    if constexpr (NT == kStoreStreamDrop) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(g, 0, bytes, 0x00020000);  // (lanes beyond it: dropped)
#pragma unroll
        for (int i = 0; i < FULL; ++i) {
            vec4u t = {v[i].x, v[i].y, v[i].z, v[i].w};
            __builtin_amdgcn_raw_buffer_store_b128(t, rs, (lane + 64 * i) * 16, 0, 2 | 16);
        }
        if (REM && lane < REM) {
            vec4u t = {v[FULL].x, v[FULL].y, v[FULL].z, v[FULL].w};
            __builtin_amdgcn_raw_buffer_store_b128(t, rs, (lane + 64 * FULL) * 16, 0, 2 | 16);
        }
        return;
    }
#endif
    constexpr int P = NT == kStoreStreamDrop ? kStoreStream : NT;
    uint4 *gv = reinterpret_cast<uint4 *>(g);
    const int nvec = bytes >> 4;
#pragma unroll
    for (int i = 0; i < FULL; ++i)
        if (lane + 64 * i < nvec) store16<P>(&gv[lane + 64 * i], v[i]);
    if (REM && lane < REM && lane + 64 * FULL < nvec) store16<P>(&gv[lane + 64 * FULL], v[FULL]);
}

// ---- sub-tiles: BPS boards per wavefront, LPB = 64 / BPS lanes per board (batches that do not fill the chip) -------------------
// A batch of a few thousand boards is a few dozen 64-board tiles: most CUs idle and a launch lasts as long as ONE wavefront's
// serial path.  The role kernels (k_collect_small) cut a tile in LPB parts: lane = LPB * board + j, the LPB lanes of a board
// compute the game (sample, move, winner, legal mask) REDUNDANTLY -- no cross-lane traffic at all -- and share the per-row work:
// lane j builds bytes [64 j / LPB, 64 (j + 1) / LPB) of the board's mask row and drops every LPB-th channel of its observation
// row, and a sub-tile's images are 1 / LPB of a tile's (16 x 117 B = 117 vectors: two store instructions instead of eight).
// LPB = 4: 16 boards per wavefront (up to 8 192 boards), 2: 32 boards (round 5), 1: a whole tile per wavefront.  Sub-tile s of an
// array of ROWB-byte rows starts at byte BPS s ROWB, a multiple of 16 like a tile.
constexpr int kSub = 16;

template <int ROWB, int BPS = kSub, typename Between = NoWork>
__device__ __forceinline__ void sub_in(const int8_t *__restrict__ g, uint32_t *lds, int lane, int rows, Between between = Between())
{
    constexpr int NV = BPS * ROWB / 16;
    static_assert(NV <= 128 && (BPS * ROWB) % 16 == 0, "at most two vectors per lane");
    if (rows == BPS) {
        const uint4 *gv = reinterpret_cast<const uint4 *>(g);
        uint4 *lv = reinterpret_cast<uint4 *>(lds);
        uint4 v[2];
        v[0] = gv[lane < NV ? lane : NV - 1];  // branch-free, like tile_in
        v[1] = gv[NV > 64 && lane + 64 < NV ? lane + 64 : NV - 1];
        between();
#ifndef GBL_HOST_EMU
        pin_loads<2>(v);
#endif
        if (lane < NV) lv[lane] = v[0];
        if (NV > 64 && lane + 64 < NV) lv[lane + 64] = v[1];
    } else {  // ragged last sub-tile: its whole vectors (clamped: nothing beyond the rows is read), then the last few bytes (tile_in)
        const int bytes = rows * ROWB, nvec = bytes >> 4;
        const uint4 *gv = reinterpret_cast<const uint4 *>(g);
        uint4 *lv = reinterpret_cast<uint4 *>(lds);
        int8_t *lb = reinterpret_cast<int8_t *>(lds);
        uint4 v[2];
        const int last = nvec > 0 ? nvec - 1 : 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) v[i] = nvec > 0 ? gv[lane + 64 * i < nvec ? lane + 64 * i : last] : uint4{0u, 0u, 0u, 0u};
        const int ti = (nvec << 4) + lane;
        const int8_t tb = ti < bytes ? g[ti] : (int8_t)0;
        between();
#pragma unroll
        for (int i = 0; i < 2; ++i)
            if (lane + 64 * i < nvec) lv[lane + 64 * i] = v[i];
        if (ti < bytes) lb[ti] = tb;
    }
}

template <int ROWB, int NT, int BPS = kSub>
__device__ __forceinline__ void sub_out(int8_t *__restrict__ g, const uint32_t *lds, int lane, int rows)
{
    constexpr int NV = BPS * ROWB / 16;
    static_assert(NV <= 128 && (BPS * ROWB) % 16 == 0, "at most two vectors per lane");
    if (rows == BPS) {
        const uint4 *lv = reinterpret_cast<const uint4 *>(lds);
        uint4 v[2];
        v[0] = lv[lane < NV ? lane : NV - 1];
        if (NV > 64) v[1] = lv[lane + 64 < NV ? lane + 64 : NV - 1];
#ifndef GBL_HOST_EMU
        if constexpr (NT == kStoreStreamDrop) {
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(g, 0, BPS * ROWB, 0x00020000);
            if (lane < NV) {
                vec4u t = {v[0].x, v[0].y, v[0].z, v[0].w};
                __builtin_amdgcn_raw_buffer_store_b128(t, rs, lane * 16, 0, 2 | 16);
            }
            if (NV > 64 && lane + 64 < NV) {
                vec4u t = {v[1].x, v[1].y, v[1].z, v[1].w};
                __builtin_amdgcn_raw_buffer_store_b128(t, rs, (lane + 64) * 16, 0, 2 | 16);
            }
            return;
        }
#endif
        constexpr int P = NT == kStoreStreamDrop ? kStoreStream : NT;
        uint4 *gv = reinterpret_cast<uint4 *>(g);
        if (lane < NV) store16<P>(&gv[lane], v[0]);
        if (NV > 64 && lane + 64 < NV) store16<P>(&gv[lane + 64], v[1]);
    } else {
        const int bytes = rows * ROWB;
        const int8_t *lb = reinterpret_cast<const int8_t *>(lds);
        for (int i = lane; i < bytes; i += 64) g[i] = lb[i];
    }
}

// A sub-tile's output image (mask / observation rows of BPS boards: up to 468 vectors) on its way out: fetched from LDS into
// registers at the end of one ply, stored behind the next ply's sample and move.  Named members, not an array: an array handed
// around by reference was "promoted" to LDS by the compiler (round 4).
template <int N>
struct SubVecs {
    uint4 head;
    SubVecs<N - 1> tail;
    template <int I>
    __device__ __forceinline__ uint4 &at()
    {
        if constexpr (I == 0) return head;
        else return tail.template at<I - 1>();
    }
};
template <>
struct SubVecs<0> {
};

template <int ROWB, int BPS>
constexpr int sub_vectors() { return (BPS * ROWB / 16 + 63) / 64; }

template <int ROWB, int BPS, int I = 0>
__device__ __forceinline__ void sub_fetch(const uint32_t *lds, int lane, SubVecs<sub_vectors<ROWB, BPS>()> &v)
{
    constexpr int NV = BPS * ROWB / 16, N = sub_vectors<ROWB, BPS>();
    if constexpr (I < N) {
        const uint4 *lv = reinterpret_cast<const uint4 *>(lds);
        const int i = lane + 64 * I;
        v.template at<I>() = lv[64 * I + 63 < NV ? i : (i < NV ? i : NV - 1)];
        sub_fetch<ROWB, BPS, I + 1>(lds, lane, v);
    }
}

// `bytes`: what of the image leaves -- BPS * ROWB for a whole sub-tile; the WHOLE 16-byte vectors of a ragged one's rows (a multiple
// of 16; its last few bytes go out with sub_tail, so that a ragged sub-tile takes the same deferred register path as a whole one:
// the launch of a latency-bound batch lasts as long as its slowest wavefront, and the ragged one used to copy its rows LDS -> HBM
// vector by vector inside the ply -- 16 447 boards 1.00 us per ply where 16 384 take 0.74 and 20 480 take 0.84).
template <int ROWB, int NT, int BPS, int I = 0>
__device__ __forceinline__ void sub_store(int8_t *__restrict__ g, SubVecs<sub_vectors<ROWB, BPS>()> &v, int lane, int bytes = BPS * ROWB)
{
    constexpr int N = sub_vectors<ROWB, BPS>();
    if constexpr (I < N) {
        const int i = lane + 64 * I;
        const uint4 &x = v.template at<I>();
#ifndef GBL_HOST_EMU
        if constexpr (NT == kStoreStreamDrop) {
            // (no predicate: the descriptor covers exactly the bytes that leave, and the hardware drops a lane whose offset lies
            //  beyond it -- the lanes past the last vector)
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(g, 0, bytes, 0x00020000);
            vec4u t = {x.x, x.y, x.z, x.w};
            __builtin_amdgcn_raw_buffer_store_b128(t, rs, i * 16, 0, 2 | 16);
        } else
#endif
        {
            constexpr int P = NT == kStoreStreamDrop ? kStoreStream : NT;
            if (16 * i + 16 <= bytes) store16<P>(reinterpret_cast<uint4 *>(g) + i, x);
        }
        sub_store<ROWB, NT, BPS, I + 1>(g, v, lane, bytes);
    }
}

// the last bytes of a ragged sub-tile's rows, behind its whole vectors (< 16 bytes: one byte per lane, from the LDS image)
__device__ __forceinline__ void sub_tail(int8_t *__restrict__ g, const uint32_t *lds, int lane, int bytes)
{
    const int i = (bytes & ~15) + lane;
    if (i < bytes) g[i] = reinterpret_cast<const int8_t *>(lds)[i];
}

// zero image of a sub-tile's BPS observation rows
template <int BPS = kSub>
__device__ __forceinline__ void sub_obs_zero(uint32_t *img, int lane)
{
    constexpr int NV = BPS * kObs / 16;
    uint4 *lv = reinterpret_cast<uint4 *>(img);
    const uint4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < (NV + 63) / 64; ++i) lv[(64 * i + 63 < NV || lane + 64 * i < NV) ? lane + 64 * i : NV - 1] = z;  // (no branch)
}

// Orders this wave's LDS accesses across lanes.  A workgroup is ONE wavefront, whose LDS
// instructions execute in issue order, so no s_barrier and no vmcnt drain is needed (a
// __syncthreads() would also wait for every outstanding global store); the fence only keeps the
// compiler from moving LDS accesses across this point.
__device__ __forceinline__ void wave_lds_fence()
{
#ifndef GBL_HOST_EMU
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#endif
}

// Workgroup barrier for kernels whose wavefronts share LDS only: waits for the caller's LDS traffic (lgkmcnt) but NOT for
// its outstanding global stores (vmcnt), which __syncthreads() would -- a wavefront's trajectory stores stay in flight
// across the rendezvous.
__device__ __forceinline__ void pair_barrier()
{
#ifndef GBL_HOST_EMU
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}

// ---- LDS image <-> one row per lane ---------------------------------------------------
// Lane l's row = image bytes [l*ROWB, (l+1)*ROWB).  r[] holds the row as
// little-endian dwords; bytes past ROWB in the last dword are unspecified.
// The image needs 4 readable bytes of slack after the tile.
template <int ROWB>
__device__ __forceinline__ void row_load(const uint32_t *lds, int lane, uint32_t (&r)[(ROWB + 3) / 4])
{
    constexpr int NW = (ROWB + 3) / 4;
    uint32_t byteoff = (uint32_t)lane * ROWB;
    uint32_t q0 = byteoff >> 2, sh = byteoff & 3u;
    uint32_t x[NW + 1];
#pragma unroll
    for (int k = 0; k <= NW; ++k) x[k] = lds[q0 + k];
#pragma unroll
    for (int k = 0; k < NW; ++k) r[k] = alignbyte(x[k + 1], x[k], sh);
}

// Each lane owns the image dwords whose FIRST byte lies in its row; the last
// owned dword may end with up to 3 bytes of the next lane's row, fetched with
// one DPP/shuffle of that lane's first dword.  64*ROWB is a multiple of 4, so
// lane 63's last dword ends exactly at the tile end.
template <int ROWB>
__device__ __forceinline__ void row_stage(uint32_t *lds, int lane, const uint32_t (&d)[(ROWB + 3) / 4])
{
    constexpr int NW = (ROWB + 3) / 4;
    constexpr int TAIL = ROWB % 4;
    static_assert(TAIL != 0, "dword-multiple rows need no shifting");
    uint32_t byteoff = (uint32_t)lane * ROWB;
    uint32_t h = (4u - (byteoff & 3u)) & 3u;  // leading bytes that belong to the previous lane's last dword
    uint32_t qfirst = (byteoff + 3u) >> 2;
    uint32_t cnt = (ROWB - h + 3u) >> 2;      // NW or NW-1
    uint32_t nd0 = __shfl_down(d[0], 1);
    uint32_t e_last = (d[NW - 1] & ((1u << (8 * TAIL)) - 1u)) | (nd0 << (8 * TAIL));
    uint32_t e_over = nd0 >> (8 * (4 - TAIL));
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        uint32_t lo = (k == NW - 1) ? e_last : d[k];
        uint32_t hi = (k + 1 == NW - 1) ? e_last : (k + 1 == NW) ? e_over : d[k + 1];
        uint32_t w = alignbyte(hi, lo, h);
        if (k < NW - 1 || cnt == NW) lds[qfirst + k] = w;
    }
}

// ---- bit planes ------------------------------------------------------------------------
struct Planes {
    uint32_t nz, neg, odd;  // 27 bits each; neg / odd are only meaningful where nz is set
};

// r[0..6] = the 27 state bytes (r[6] byte 3 ignored).  Exact per-byte tests in
// SWAR, then v_dot4_u32_u8 with weights (1,2,4,8 | 16,32,64,128) gathers one
// flag bit per byte of two dwords into 8 contiguous bits.
__device__ __forceinline__ Planes make_planes(const uint32_t (&r)[7])
{
    Planes p{0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 7; j += 2) {
        uint32_t anz = 0, ang = 0, aod = 0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (j + u >= 7) break;
            uint32_t x = r[j + u];
            if (j + u == 6) x &= 0x00FFFFFFu;
            uint32_t w = u ? 0x80402010u : 0x08040201u;
            uint32_t t = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;  // 0x80 where byte != 0
            anz = __builtin_amdgcn_udot4(t, w, anz, false);
            ang = __builtin_amdgcn_udot4(x & 0x80808080u, w, ang, false);
            aod = __builtin_amdgcn_udot4(x & 0x01010101u, w, aod, false);
        }
        p.nz |= (anz >> 7) << (4 * j);
        p.neg |= (ang >> 7) << (4 * j);
        p.odd |= aod << (4 * j);
    }
    return p;
}

// Board.check_for_winner, board.py:183-194, over the tops of get_flatboard
// (board.py:159-177).  The reference walks the 8 lines in a fixed order with no
// early exit, so the matching line with the HIGHEST index decides; one line
// cannot match both colours, so comparing the two 8-bit match masks as
// integers picks that line's colour.
//
// line_matches: the 8-bit mask of the lines (bit l = line l of board.py:135-153) on which every top piece is `colour`'s
// (0 = player_1).  side = the colour's cells (nz & ~neg / nz & neg), passed in so that a caller whose lanes split the two colours
// selects it with one operation.
__device__ __forceinline__ uint32_t line_matches_of(uint32_t side, uint32_t nz)
{
    uint32_t o1 = (nz >> 9) & 0x1FFu, o2 = (nz >> 18) & 0x1FFu;
    uint32_t t = ((side >> 18) & 0x1FFu) | (~o2 & (((side >> 9) & 0x1FFu) | (~o1 & (side & 0x1FFu))));  // the colour's tops
    // board.py:135-153: (0,1,2) (3,4,5) (6,7,8) (0,3,6) (1,4,7) (2,5,8) (0,4,8) (2,4,6).
    // Three lines per word in 10-bit fields (bit 9 = guard): adding 0x1FF to "squares of the line the
    // side lacks" carries into the guard iff something is missing.  Lines (0,3,6) / (1,4,7) / (2,5) share
    // a word so that shifting the guards by 9 / 8 / 7 lays the eight match bits out in line order.
    constexpr uint32_t L[8] = {0x007u, 0x038u, 0x1C0u, 0x049u, 0x092u, 0x124u, 0x111u, 0x054u};
    constexpr uint32_t LOW3 = 0x00100401u, G3 = LOW3 << 9, F3 = LOW3 * 0x1FFu;
    constexpr uint32_t WA = L[0] | (L[3] << 10) | (L[6] << 20), WB = L[1] | (L[4] << 10) | (L[7] << 20);
    constexpr uint32_t WC = L[2] | (L[5] << 10), NONE = 1u << 20;  // third field of WC: always "missing"
    uint32_t n = ~(t | (t << 10) | (t << 20));
    return ((G3 & ~((WA & n) + F3)) >> 9) | ((G3 & ~((WB & n) + F3)) >> 8) | ((G3 & ~(((WC & n) | NONE) + F3)) >> 7);
}

__device__ __forceinline__ int winner_from_matches(uint32_t m1, uint32_t m2) { return m2 > m1 ? -1 : (m1 > m2 ? 1 : 0); }

__device__ __forceinline__ int winner_of(const Planes &p)
{
    return winner_from_matches(line_matches_of(p.nz & ~p.neg, p.nz), line_matches_of(p.nz & p.neg, p.nz));
}

// winner_of for kernels whose lanes come in PAIRS that hold the same board (the role kernels with two or four lanes per board):
// the even lane of a pair walks player_1's lines, the odd lane player_2's, and one DPP quad permutation ([1, 0, 3, 2]) hands
// each the other's match mask -- half the line arithmetic per lane (~28 instead of ~48 instructions on the ply's serial chain).
// j = the lane's index among its board's lanes (only its parity is used).  The host emulation, whose lanes run one after the
// other, computes both masks itself: the same function of the same board.
__device__ __forceinline__ int winner_of_pair(const Planes &p, int j)
{
#ifndef GBL_HOST_EMU
    const uint32_t flip = (j & 1) ? 0u : ~0u;                                     // (a per-lane constant)
    const uint32_t mine = line_matches_of(p.nz & (p.neg ^ flip), p.nz);           // colour j & 1
    const uint32_t theirs = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0xB1, 0xf, 0xf, false);  // quad_perm [1, 0, 3, 2]
    const int w = mine > theirs ? 1 : (theirs > mine ? -1 : 0);                   // seen from colour j & 1
    return (j & 1) ? -w : w;
#else
    (void)j;
    return winner_of(p);
#endif
}

// 54-bit legal mask of agent `mover` (0 / 1): raw_env._legal_moves,
// gobblet.py:223-228 = 54 x Board.is_legal, board.py:82-115.
//   mask[9*piece + pos] = piece not covered (board.py:90-102, check_covered :203-220)
//                         and size(piece) > size(top at pos) (board.py:106-115)
__device__ __forceinline__ uint64_t legal54(const Planes &p, int mover)
{
    uint32_t o0 = p.nz & 0x1FFu, o1 = (p.nz >> 9) & 0x1FFu, o2 = (p.nz >> 18) & 0x1FFu;
    uint32_t cov = (o0 & (o1 | o2)) | ((o1 & o2) << 9);  // covered cells (levels 0,1)
    uint32_t mine = mover ? (p.nz & p.neg) : (p.nz & ~p.neg);
    uint32_t bl = mine & cov;
    uint32_t blo = bl & p.odd, ble = bl & ~p.odd;
    uint32_t ok0 = ~(o0 | o1 | o2) & 0x1FFu, ok1 = ~(o1 | o2) & 0x1FFu, ok2 = ~o2 & 0x1FFu;
    uint32_t g0 = (blo & 0x1FFu) ? 0u : ok0;      // piece 1
    uint32_t g1 = (ble & 0x1FFu) ? 0u : ok0;      // piece 2
    uint32_t g2 = (blo & 0x3FE00u) ? 0u : ok1;    // piece 3
    uint32_t g3 = (ble & 0x3FE00u) ? 0u : ok1;    // piece 4
    uint32_t lo = g0 | (g1 << 9) | (g2 << 18) | (g3 << 27);
    uint32_t hi = (g3 >> 5) | (ok2 << 4) | (ok2 << 13);  // pieces 5, 6 are never covered
    return ((uint64_t)hi << 32) | lo;
}

// Board.play_turn(mover, a), board.py:118-132, given that `a` is legal: clear the cell holding the
// piece (if placed), write it at 9*level + pos.  The planes are updated here; the two cells of the
// 27-byte row that change are returned for whoever holds the row.
struct MoveCells {
    uint32_t cold, cnew, val;  // cell to clear (only if `had`), cell to write, signed piece number as a byte
    bool had;                  // the piece was on the board already
};

__device__ __forceinline__ MoveCells move_planes(Planes &p, int mover, uint32_t a)
{
    // a / 9 for a < 54 through a 24-bit multiply (full rate; the compiler turns __umul24 back into the quarter-rate v_mul_lo_u32
    // wherever it cannot bound `a`, hence the instruction by name)
#ifndef GBL_HOST_EMU
    uint32_t a57;
    asm("v_mul_u32_u24 %0, %1, 57" : "=v"(a57) : "v"(a));
    uint32_t pi = a57 >> 9;
#else
    uint32_t pi = (a * 57u) >> 9;
#endif
    uint32_t q = a - 9u * pi;
    uint32_t k = pi >> 1;
    uint32_t first = (~pi) & 1u;   // piece number odd
    uint32_t mine = mover ? (p.nz & p.neg) : (p.nz & ~p.neg);
    uint32_t ploc = mine & (first ? p.odd : ~p.odd) & (0x1FFu << (9u * k));
    uint32_t cnew = 9u * k + q, bit = 1u << cnew;
    p.nz = (p.nz & ~ploc) | bit;
    p.neg = (p.neg & ~ploc & ~bit) | (mover ? bit : 0u);
    p.odd = (p.odd & ~ploc & ~bit) | (first ? bit : 0u);
    MoveCells m;
    m.had = ploc != 0;
    m.cold = m.had ? (uint32_t)__builtin_ctz(ploc) : 0u;
    m.cnew = cnew;
    m.val = (mover ? (0u - (pi + 1u)) : (pi + 1u)) & 0xFFu;
    return m;
}

// No row: a wavefront that plays the game without writing the state back (the role kernels' row wavefronts) patches nothing.
struct NoRow {
    __device__ __forceinline__ void apply(const MoveCells &) const {}
    __device__ __forceinline__ void reset() const {}
};

// The row in 7 registers (board-level kernels: the row is re-staged into a fresh image anyway).
struct RegRow {
    uint32_t (&r)[7];
    __device__ __forceinline__ void apply(const MoveCells &m)
    {
        uint32_t cold = m.had ? m.cold : 63u * 4u;
        uint32_t mold = ~(0xFFu << (8u * (cold & 3u)));
        uint32_t mnew = ~(0xFFu << (8u * (m.cnew & 3u)));
        uint32_t vnew = m.val << (8u * (m.cnew & 3u));
#pragma unroll
        for (uint32_t j = 0; j < 7; ++j) {
            uint32_t x = r[j];
            x = (j == (cold >> 2)) ? (x & mold) : x;
            x = (j == (m.cnew >> 2)) ? ((x & mnew) | vnew) : x;
            r[j] = x;
        }
    }
    __device__ __forceinline__ void reset()
    {
#pragma unroll
        for (int j = 0; j < 7; ++j) r[j] = 0;
    }
};

// The row where the tile load put it, in the LDS image (step kernels: the image goes back out as it
// is, so a move costs two byte stores and a reset one 27-byte clear instead of rebuilding and
// re-staging 7 dwords).  Rows are 27 bytes apart: the clear relies on unaligned LDS stores (gfx950).
struct ImageRow {
    uint8_t *row;
    __device__ __forceinline__ void apply(const MoveCells &m) const
    {
        // (no branch: a piece that comes from the hand clears the cell it is about to fill -- LDS stores of a lane land in order)
        row[m.had ? m.cold : m.cnew] = 0;
        row[m.cnew] = (uint8_t)m.val;
    }
    __device__ __forceinline__ void reset() const { __builtin_memset(row, 0, kCells); }
};

__device__ __forceinline__ void apply_move(Planes &p, uint32_t (&r)[7], int mover, uint32_t a)
{
    RegRow{r}.apply(move_planes(p, mover, a));
}

// The 27 state bytes of a board from its planes (the inverse of make_planes on contract states: a level-k cell holds 0 or
// +-(2k+1), +-(2k+2)): a kernel that plays many plies on the planes alone writes the state back ONCE, from here, instead of
// patching a byte row every ply (k_collect5).  r[6]'s top byte is 0.
__device__ __forceinline__ void planes_to_row(const Planes &p, uint32_t (&r)[7])
{
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        uint32_t w = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = 4 * j + u;
            if (c < kCells) {
                const int k = c / 9;
                const uint32_t nz = (p.nz >> c) & 1u, ng = (p.neg >> c) & nz, od = (p.odd >> c) & nz;
                const uint32_t v = nz * (uint32_t)(2 * k + 2) - od;   // 2k+2, or 2k+1 where the piece number is odd; 0 where empty
                w |= (ng ? (0u - v) & 0xFFu : v) << (8 * u);
            }
        }
        r[j] = w;
    }
}

// ---- row encoders ----------------------------------------------------------------------
// 54 mask bits -> 54 bytes of 0/1 (14 dwords; bytes 54,55 are zero)
__device__ __forceinline__ void mask_row(uint64_t m, uint32_t (&d)[14])
{
    uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
#pragma unroll
    for (int j = 0; j < 14; ++j) {
        uint32_t nib = ((j < 8 ? lo : hi) >> (4 * (j & 7))) & 0xFu;
        d[j] = __umul24(nib, 0x00204081u) & 0x01010101u;  // bit i -> byte i
    }
}

// raw_env.observe, gobblet.py:179-208: obs[pos][ch], int8[9][13]:
//   ch 0..5 : cell(level ch/2, pos) == +(ch+1) seen from the observer (own pieces)
//   ch 6..11: cell(level (ch-6)/2, pos) == -(ch-5)                     (opponent's)
//   ch 12   : the observer's agent index
// written SPARSELY into a tile's LDS image: an observation has at most 12
// ones among channels 0..11 (one per piece on the board) plus the 9 bytes of channel 12, so instead
// of composing 30 dwords per board (~2 VALU per byte) the wave zero-fills the image with
// 16-byte stores and every lane then drops single bytes at  lane*117 + 13*pos + ch  -- one
// predicated ds_write_b8 per piece.  Relies on the state contract (a piece number occurs at most
// once), like everything else.  Call obs_image_zero, fence, obs_scatter, fence, tile_out.
__device__ __forceinline__ void obs_image_zero(uint32_t *img, int lane)
{
    constexpr int NV = kTile * kObs / 16, FULL = NV / 64, REM = NV % 64;
    uint4 *lv = reinterpret_cast<uint4 *>(img);
    const uint4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < FULL; ++i) lv[lane + 64 * i] = z;
    if (REM && lane < REM) lv[lane + 64 * FULL] = z;
}

__device__ __forceinline__ void obs_scatter_row(uint8_t *row, const Planes &p, int observer);

__device__ __forceinline__ void obs_scatter(uint32_t *img, int lane, const Planes &p, int observer)
{
    obs_scatter_row(reinterpret_cast<uint8_t *>(img) + lane * kObs, p, observer);
}

// row: the board's 117 observation bytes, zero on entry.  Straight-line code: a piece that is not on the board writes a 0 to square
// 8 of its own channel, which no other piece can set, and channel 12 is written whoever observes (round 5: the predicated form --
// one EXEC round trip per piece -- cost the latency-bound kernels 10-15 % of a ply; the HBM-bound ones do not care, +-1-2 %).
__device__ __forceinline__ void obs_scatter_row(uint8_t *row, const Planes &p, int observer)
{
    uint32_t pos = p.nz & ~p.neg, ngv = p.nz & p.neg;
    uint32_t own = observer ? ngv : pos, opp = observer ? pos : ngv;
    uint32_t X[4] = {own & p.odd, own & ~p.odd, opp & p.odd, opp & ~p.odd};  // A B C D
#pragma unroll
    for (int ch = 0; ch < 12; ++ch) {
        int k = (ch % 6) / 2;
        uint32_t grp = (X[(ch < 6 ? 0 : 2) + (ch & 1)] >> (9 * k)) & 0x1FFu;
        row[13 * __builtin_ctz(grp | 0x100u) + ch] = (uint8_t)(grp ? 1u : 0u);
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) row[13 * q + 12] = (uint8_t)observer;
}

// Lane j (of the LPB of a board) drops channels j, j + LPB, ... and the channel-12 bytes of squares j, j + LPB, ... of the board's
// observation row (zero on entry): obs_scatter_row dealt over the board's lanes.
template <int LPB = 4>
__device__ __forceinline__ void obs_scatter_part(uint8_t *row, const Planes &p, int observer, int j)
{
    static_assert(LPB == 1 || LPB == 2 || LPB == 4, "lanes per board");
    if constexpr (LPB == 1) {
        (void)j;
        obs_scatter_row(row, p, observer);
    } else {
        // STRAIGHT-LINE code (the role kernels' wavefronts run alone on their SIMDs: a predicated region costs them its EXEC
        // round trips, not its instructions): a piece that is not on the board writes a 0 to square 8 of its own channel, which
        // no other piece can set; a channel-12 byte past square 8 is redirected to the lane's first square (the same value again).
        const uint32_t pos = p.nz & ~p.neg, ngv = p.nz & p.neg;
        const uint32_t own = observer ? ngv : pos, opp = observer ? pos : ngv;
        // channel ch = j + LPB i: side = ch / 6, level = (ch % 6) / 2, parity = ch & 1 = j & 1 (LPB is even)
        const uint32_t oddsel = (j & 1) ? ~p.odd : p.odd;
        const uint32_t ownsel = own & oddsel, oppsel = opp & oddsel;
#pragma unroll
        for (int i = 0; i < 12 / LPB; ++i) {
            const int ch = j + LPB * i;                  // 0..11
            const uint32_t side = ch >= 6 ? oppsel : ownsel;
            const int k = (ch >= 6 ? ch - 6 : ch) >> 1;
            const uint32_t grp = (side >> (9 * k)) & 0x1FFu;
            row[13 * __builtin_ctz(grp | 0x100u) + ch] = (uint8_t)(grp ? 1u : 0u);
        }
#pragma unroll
        for (int i = 0; i < (9 + LPB - 1) / LPB; ++i) {
            const int q = j + LPB * i;
            row[13 * (q < 9 ? q : j) + 12] = (uint8_t)observer;
        }
    }
}

__device__ __forceinline__ void obs_scatter_quad(uint8_t *row, const Planes &p, int observer, int j)
{
    obs_scatter_part<4>(row, p, observer, j);
}

// Lane j writes S = 64 / LPB bytes of the board's 54-byte mask row at `row` -- bytes [S j, S j + S), the last lane the LAST S
// bytes of the row (it overlaps its neighbour's share with the same values: no branch, see obs_scatter_part); one lane per board:
// all 54.  Rows are 2-byte aligned: unaligned LDS stores, like ImageRow::reset.
template <int LPB = 4>
__device__ __forceinline__ void mask_row_part(uint8_t *row, uint64_t m, int j)
{
    static_assert(LPB == 1 || LPB == 2 || LPB == 4, "lanes per board");
    constexpr int S = 64 / LPB, NW = S / 4;  // bytes per lane, dwords per lane
    const int first = LPB == 1 ? 0 : (S * j < kActions - S ? S * j : kActions - S);  // the lane's first byte (= bit of m)
    const uint64_t part = LPB == 1 ? m : (m >> first);
    uint32_t d[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const uint32_t nib = (uint32_t)(part >> (4 * k)) & 0xFu;
        d[k] = __umul24(nib, 0x00204081u) & 0x01010101u;  // bit i -> byte i
    }
    if constexpr (LPB == 1) __builtin_memcpy(row, d, kActions);
    else __builtin_memcpy(row + first, d, S);
}

__device__ __forceinline__ void mask_row_quad(uint8_t *row, uint64_t m, int j) { mask_row_part<4>(row, m, j); }

// Board.get_flatboard, board.py:159-177: signed piece number of the top piece per
// square, as a 9-byte row in 3 dwords.
__device__ __forceinline__ void flat_row(const Planes &p, const uint32_t (&r)[7], uint32_t (&d)[3])
{
    uint32_t o1 = (p.nz >> 9) & 0x1FFu, o2 = (p.nz >> 18) & 0x1FFu;
    d[0] = d[1] = d[2] = 0;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        uint32_t b0 = (r[q >> 2] >> (8 * (q & 3))) & 0xFFu;
        uint32_t b1 = (r[(9 + q) >> 2] >> (8 * ((9 + q) & 3))) & 0xFFu;
        uint32_t b2 = (r[(18 + q) >> 2] >> (8 * ((18 + q) & 3))) & 0xFFu;
        uint32_t v = ((o2 >> q) & 1u) ? b2 : (((o1 >> q) & 1u) ? b1 : b0);
        d[q >> 2] |= v << (8 * (q & 3));
    }
}

// Board.check_covered, board.py:203-220: 27 bytes of 0/1 in 7 dwords.
__device__ __forceinline__ void covered_row(const Planes &p, uint32_t (&d)[7])
{
    uint32_t o0 = p.nz & 0x1FFu, o1 = (p.nz >> 9) & 0x1FFu, o2 = (p.nz >> 18) & 0x1FFu;
    uint32_t cov = (o0 & (o1 | o2)) | ((o1 & o2) << 9);
#pragma unroll
    for (int j = 0; j < 7; ++j) d[j] = __umul24((cov >> (4 * j)) & 0xFu, 0x00204081u) & 0x01010101u;
}

// State-contract check (not on the hot path): bit 0 = some cell of level k holds a value other than
// 0, +-(2k+1), +-(2k+2); bit 1 = some piece number occurs twice -- the condition on which the
// reference raises Exception("PIECE HAS BEEN USED TWICE") (board.py:94-95).
__device__ __forceinline__ uint32_t validate_row(const uint32_t (&r)[7])
{
    uint32_t bad = 0;
#pragma unroll
    for (int c = 0; c < kCells; ++c) {
        int v = (int)(int8_t)((r[c >> 2] >> (8 * (c & 3))) & 0xFFu);
        int a = v < 0 ? -v : v, k = c / 9;
        bad |= (v != 0 && a != 2 * k + 1 && a != 2 * k + 2) ? 1u : 0u;
    }
    Planes p = make_planes(r);
    uint32_t pos = p.nz & ~p.neg, ngv = p.nz & p.neg;
    uint32_t X[4] = {pos & p.odd, pos & ~p.odd, ngv & p.odd, ngv & ~p.odd};
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int k = 0; k < 3; ++k) bad |= (__popc((X[g] >> (9 * k)) & 0x1FFu) > 1) ? 2u : 0u;
    return bad;
}

// ---- Philox4x32-10 (Salmon et al., SC'11); known answers are checked in tests/ ---------------
struct Draw4 {
    uint32_t w[4];
};

__device__ __forceinline__ Draw4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                               uint32_t k1)
{
#pragma unroll
    for (int rnd = 0; rnd < 10; ++rnd) {
        // one 32 x 32 -> 64 multiply per product (v_mad_u64_u32: 2.9 cycles of SIMD time at full occupancy, the
        // same as v_mul_hi_u32 or v_mul_lo_u32 alone -- scripts/microbench/valu_rates.hip) instead of two
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Draw4{{c0, c1, c2, c3}};
}

// index of the k-th (0-based) set bit of w; k < popcount(w)
__device__ __forceinline__ uint32_t kth_bit32(uint32_t w, uint32_t k)
{
    uint32_t pos = 0;
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) {
        uint32_t c = __popc(w & ((1u << s) - 1u));
        bool up = k >= c;
        k = up ? k - c : k;
        w = up ? (w >> s) : w;
        pos += up ? s : 0;
    }
    return pos;
}

// masked-uniform draw (see gbl_sample in include/gobblet_hip.h), in two halves: the 32-bit draw
// depends only on (seed, board id, ply) -- a kernel can compute it while its tile is still in
// flight -- and the pick needs the mask.  One Philox block serves four consecutive plies of a board
// (word ply & 3 of the block with counter ply >> 2): a kernel that plays several plies per launch
// runs the generator once per four.
// `stream` (counter word 3) separates the consumers of one (seed, board) pair: kStreamEnv = the masked-random
// actions of gbl_sample / gbl_rollout, kStreamGreedy = the greedy policy's fallback draw (gbl_greedy_act),
// kStreamPlayout = the moves of the Monte-Carlo playouts (gbl_playout_values, keyed by a playout id, not a board id).
constexpr uint32_t kStreamEnv = 0u, kStreamGreedy = 1u, kStreamPlayout = 2u;

__device__ __forceinline__ Draw4 draw_block(uint64_t seed, uint64_t env_id, uint32_t ply, uint32_t stream = kStreamEnv)
{
    return philox4x32_10((uint32_t)env_id, (uint32_t)(env_id >> 32), ply >> 2, stream, (uint32_t)seed,
                         (uint32_t)(seed >> 32));
}

__device__ __forceinline__ uint32_t draw_word(const Draw4 &d, uint32_t ply)
{
    uint32_t lo = (ply & 1u) ? d.w[1] : d.w[0], hi = (ply & 1u) ? d.w[3] : d.w[2];
    return (ply & 2u) ? hi : lo;
}

// which word of the block draw_word picks: ply & 3 = 0, 1, 2, 3 -> w[0], w[1], w[2], w[3]
__device__ __forceinline__ uint32_t draw_word_index(uint32_t ply) { return ply & 3u; }

__device__ __forceinline__ uint32_t draw32(uint64_t seed, uint64_t env_id, uint32_t ply, uint32_t stream = kStreamEnv)
{
    return draw_word(draw_block(seed, env_id, ply, stream), ply);
}

// legal54 of the empty board, for either mover: every piece on every cell (what a reset leaves; the kernels that live on a
// lone wavefront's latency take the legal mask of the moved position BESIDE the winner test and swap this in on a reset)
constexpr uint64_t kLegalEmpty = (1ull << kActions) - 1ull;

__device__ __forceinline__ int pick54(uint64_t m, uint32_t r)
{
    uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
    uint32_t nlo = __popc(lo), n = nlo + __popc(hi);
    uint32_t k = __umulhi(r, n);
    bool low = k < nlo;  // pick the word first: one bit search instead of two
    int a = (int)kth_bit32(low ? lo : hi, low ? k : k - nlo) + (low ? 0 : 32);
    return n ? a : -1;
}

__device__ __forceinline__ int sample54(uint64_t m, uint64_t seed, uint64_t env_id, uint32_t ply)
{
    return pick54(m, draw32(seed, env_id, ply));
}

// ---- one ply of one board: raw_env.step bookkeeping, gobblet.py:231-271 -------------------
constexpr int kIllegalNoop = 0;       // GBL_ILLEGAL_NOOP
constexpr int kIllegalTerminate = 1;  // GBL_ILLEGAL_TERMINATE

struct Ply {
    int winner;     // check_for_winner() after the move
    int r0, r1;     // rewards of player_1 / player_2 for this step
    bool terminal;  // the episode ended on this step
    bool stepped;   // raw_env.step ran, i.e. the reference did `self.turn += 1` (gobblet.py:270)
    bool ok;        // the action was a legal move of the mover and was played (false: illegal or outside [0, 54) -- action_status)
};

// The status byte of an externally supplied action (gbl_step_ex / gbl_collect_from_ex; include/gobblet_hip.h GBL_STATUS_*):
// bit 0 = not a legal move of the mover (the reference's silent no-op, board.py:125-126, or TerminateIllegalWrapper's case),
// bit 1 = outside [0, 54) (where the reference's env() asserts: AssertOutOfBoundsWrapper, gobblet.py:110-117).
__device__ __forceinline__ int action_status(bool ok, int action)
{
    return (ok ? 0 : 1) | ((uint32_t)action < (uint32_t)kActions ? 0 : 2);
}

// ... of an action against the mover's legal mask (the test play_ply makes)
__device__ __forceinline__ int action_status_of(uint64_t legal, int action)
{
    return action_status((uint32_t)action < (uint32_t)kActions && ((legal >> (action & 63)) & 1ull), action);
}

// TRUSTED: the action comes from pick54 on `legal` itself (the masked-random sampler inside a T-plies-per-launch kernel): it is
// legal by construction, or -1 where a board has no legal move at all (none in the game: only outside the state contract) -- the
// legality test and the illegal-action branch leave the ply's serial chain.  PAIR > 0: winner_of_pair with j = pair_j.
template <bool TRUSTED = false, bool PAIR = false, typename Row>
__device__ __forceinline__ Ply play_ply(Planes &p, Row row, int &mover, uint64_t legal, int action, int illegal_mode, int pair_j = 0)
{
    Ply y{0, 0, 0, false, false};
    bool ok = TRUSTED ? action >= 0 : ((uint32_t)action < (uint32_t)kActions && ((legal >> (action & 63)) & 1ull));
    y.ok = ok;
    if (!TRUSTED && !ok && illegal_mode == kIllegalTerminate) {
        // gobblet.py:50-51, :114: mover -1, the other 0, everyone terminated, board untouched
        y.r0 = mover ? 0 : -1;
        y.r1 = mover ? -1 : 0;
        y.terminal = true;
        return y;
    }
    y.stepped = true;
    // gobblet.py:244 (illegal: silent no-op, board.py:125-126).  (Straight-line for the role kernel's row-less wavefronts -- the
    // planes masked instead of the EXEC round trip: no effect, profiles/r05/ab_legal_ahead.txt)
    if (ok) row.apply(move_planes(p, mover, (uint32_t)action));
    mover ^= 1;                                          // gobblet.py:246,267
    y.winner = PAIR ? winner_of_pair(p, pair_j) : winner_of(p);  // gobblet.py:248-249
    y.r0 = y.winner;                                     // gobblet.py:253-260
    y.r1 = -y.winner;
    y.terminal = y.winner != 0;                          // gobblet.py:263
    return y;
}

// Lane body of gbl_step: raw_env.step + the state the next observe() is taken from.
// In: row (RegRow / ImageRow) / p (its planes) / mover / was_done / action.  Out: row, p (after the
// step), mover, dn, y.
template <typename Row>
__device__ __forceinline__ void step_lane(Row row, Planes &p, int &mover, int was_done, int action, int illegal_mode,
                                          int auto_reset, int &dn, Ply &y)
{
    y = Ply{0, 0, 0, false, false};
    dn = was_done;
    if (was_done) {
        y.ok = true;              // (no action is consumed)
        y.winner = winner_of(p);  // frozen board (reference: _was_dead_step, gobblet.py:232-236): standing result
    } else {
        y = play_ply(p, row, mover, legal54(p, mover), action, illegal_mode);
        dn = y.terminal ? 1 : 0;
        if (y.terminal && auto_reset) {  // raw_env.reset, gobblet.py:275-290
            p = Planes{0u, 0u, 0u};
            mover = 0;
            row.reset();
        }
    }
}

// raw_env.turn of one board after a ply (gobblet.py:270 `self.turn += 1`, :289 reset to 0)
__device__ __forceinline__ int next_turn(int turn, const Ply &y, int auto_reset)
{
    turn += y.stepped ? 1 : 0;
    return (y.terminal && auto_reset) ? 0 : turn;
}

// gobblet.py:209: the mask belongs to the agent to move; a frozen board has nobody to move
__device__ __forceinline__ uint64_t next_mask(const Planes &p, int mover, int dn, int auto_reset)
{
    return (dn && !auto_reset) ? 0ull : legal54(p, mover);
}

// ---- gbl_playout_values: flat Monte-Carlo playouts -------------------------------------------
// Playout k of action a on global board g draws from generator id playout_id(g, a, k) on stream kStreamPlayout, with
// ply index (call << 8) | t for its ply t (t = 0 is the root move, t = 1 .. max_plies the masked-random plies).  The id
// does not depend on the number of playouts, so the first k playouts of a board are the same for every K >= k.
__device__ __forceinline__ uint64_t playout_id(uint64_t g, uint32_t a, uint32_t k) { return (g * kActions + a) * 65536ull + k; }
__device__ __forceinline__ uint32_t playout_ply_index(uint32_t call, uint32_t t) { return (call << 8) | t; }

// One ply of a playout: the root move a0 at t = 0, else the masked-uniform move of the side to move on generator word w
// (draw_word of the block of ply index playout_ply_index(call, t)).  Returns the winner after the move, or kPlayoutStuck
// when the side to move has no legal move (nothing is played; only outside the state contract).
constexpr int kPlayoutStuck = 2;

__device__ __forceinline__ int playout_ply(Planes &p, int &side, uint32_t t, int a0, uint32_t w)
{
    const int a = t == 0 ? a0 : pick54(legal54(p, side), w);
    if (a < 0) return kPlayoutStuck;
    move_planes(p, side, (uint32_t)a);
    side ^= 1;
    return winner_of(p);
}

// The end of a playout after ply t returned w: +1 / -1 = won / lost from the root mover's side, 0 = unfinished, and the
// plies the playout played (its root move included).  done = false: the playout goes on with ply t + 1.
struct PlayoutEnd {
    bool done;
    int outcome;
    uint32_t plies;
};

__device__ __forceinline__ PlayoutEnd playout_end(int w, uint32_t t, int mover, uint32_t max_plies)
{
    if (w == kPlayoutStuck) return PlayoutEnd{true, 0, t};
    if (w != 0) return PlayoutEnd{true, mover ? -w : w, t + 1};
    return PlayoutEnd{t >= max_plies, 0, t + 1};
}

// One whole playout, ply after ply (the host flavour; the kernel interleaves the same plies with refills, k_playout)
__device__ __forceinline__ PlayoutEnd playout(const Planes &root, int mover, int a, uint64_t seed, uint64_t pid, uint32_t call,
                                              uint32_t max_plies)
{
    Planes p = root;
    int side = mover;
    Draw4 d{};
    for (uint32_t t = 0;; ++t) {
        if ((t & 3u) == 0) d = draw_block(seed, pid, playout_ply_index(call, t), kStreamPlayout);  // one block per four plies
        const PlayoutEnd e = playout_end(playout_ply(p, side, t, a, draw_word(d, t)), t, mover, max_plies);
        if (e.done) return e;
    }
}

// gbl_playout_values' decision: the candidate with the largest wins - losses, the lowest index on ties, -1 if none.  playout_key is the
// order key of a candidate (0 stands for a non-candidate): larger is better, the max over the 54 keys decides.
__device__ __forceinline__ uint32_t playout_key(int wins, int losses, int a)
{
    return ((uint32_t)(wins - losses + 8192) << 6) | (uint32_t)(63 - a);  // |wins - losses| <= 4096
}
__device__ __forceinline__ int playout_action_of(uint32_t best_key) { return best_key ? 63 - (int)(best_key & 63u) : -1; }

// 54 mask bytes (14 dwords, row_load order) -> 54 bits
__device__ __forceinline__ uint64_t mask_bits(const uint32_t (&d)[14])
{
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 14; j += 2) {
        uint32_t acc = 0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            uint32_t x = d[j + u];
            if (j + u == 13) x &= 0x0000FFFFu;
            uint32_t t = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
            acc = __builtin_amdgcn_udot4(t, u ? 0x80402010u : 0x08040201u, acc, false);
        }
        uint32_t bits8 = acc >> 7;
        if (j < 8) lo |= bits8 << (4 * j);
        else hi |= bits8 << (4 * (j - 8));
    }
    return ((uint64_t)hi << 32) | lo;
}

// GreedyGobbletPolicy board decode, greedy_policy.py:43-71: 117 obs bytes -> 27 state bytes + agent index
__device__ __forceinline__ int decode_obs_row(const uint32_t (&d)[30], uint32_t (&r)[7])
{
    auto ob = [&](int idx) -> int { return (int)(int8_t)((d[idx >> 2] >> (8 * (idx & 3))) & 0xFFu); };
    int agent = 0;
#pragma unroll
    for (int q = 0; q < 9; ++q) agent = ob(13 * q + 12) > agent ? ob(13 * q + 12) : agent;  // obs[...,12].max()
#pragma unroll
    for (int j = 0; j < 7; ++j) r[j] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            int i = 2 * k;
            int bp = (i + 1) * ob(13 * q + i) + (i + 2) * ob(13 * q + i + 1);          // :44-49
            int bo = (i + 1) * ob(13 * q + 6 + i) + (i + 2) * ob(13 * q + 6 + i + 1);  // :50-56
            int v = bp > bo ? bp : -bo;                                                // :57
            if (agent == 1) v = -v;                                                    // :67-68
            int c = 9 * k + q;
            r[c >> 2] |= ((uint32_t)v & 0xFFu) << (8 * (c & 3));
        }
    return agent;
}

// ---- GreedyGobbletPolicy.compute_action, greedy_policy.py:38-221 (depth 1 / 2 / 3) ------------
// planes-only form of apply_move (no byte row to maintain)
__device__ __forceinline__ Planes moved(const Planes &p0, int mover, uint32_t a)
{
    Planes p = p0;
    uint32_t pi = (a * 57u) >> 9, q = a - 9u * pi, k = pi >> 1, first = (~pi) & 1u;
    uint32_t mine = mover ? (p.nz & p.neg) : (p.nz & ~p.neg);
    uint32_t ploc = mine & (first ? p.odd : ~p.odd) & (0x1FFu << (9u * k));
    uint32_t bit = 1u << (9u * k + q);
    p.nz = (p.nz & ~ploc) | bit;
    p.neg = (p.neg & ~ploc & ~bit) | (mover ? bit : 0u);
    p.odd = (p.odd & ~ploc & ~bit) | (first ? bit : 0u);
    return p;
}

struct GreedyResult {
    int chosen;      // chosen_action just before the fallback test (:211), -1 = None
    uint64_t cands;  // actions_depth1 as a 54-bit set
    bool fallback;   // the reference would call np.random.choice(actions_depth1)
};

// Outcome of EVERY move of `mover` on board p at once: bit a of `win` / `lose` is set iff
// check_for_winner() after play_turn(mover, a) is the mover's / the other side's value
// (board.py:118-132 then :183-194).  Only meaningful for legal a -- the caller masks with legal54.
//
// Bit-parallel over the 9 destinations of a piece, and SWAR over three pieces at a time (10-bit fields
// of a 32-bit word, bit 9 of each field a guard): lifting a piece from its square s exposes what
// lies beneath (tops after the lift: Tm, To); dropping it on q sets the mover's top at q and clears
// the other side's.  Line l is then complete for the mover iff q supplies its only missing square
// (or nothing is missing), and stays complete for the other side iff it was complete and q is not
// on it.  The reference lets the LAST matching line decide, so lines are resolved from index 7 down,
// each destination taking the first verdict it meets.
//
// QUIET: the caller guarantees that neither side holds a complete line on p (check_for_winner() == 0).
// A lift never adds a top piece of the mover, so no line can then be complete for the mover before the
// drop, and the "nothing missing" term is dropped.
//
template <bool QUIET = false>
__device__ __forceinline__ void outcomes54(const Planes &p, int mover, uint64_t &win, uint64_t &lose)
{
    uint32_t mine = mover ? (p.nz & p.neg) : (p.nz & ~p.neg);
    uint32_t othr = mover ? (p.nz & ~p.neg) : (p.nz & p.neg);
    uint32_t m0 = mine & 0x1FFu, m1 = (mine >> 9) & 0x1FFu, m2 = (mine >> 18) & 0x1FFu;
    uint32_t t0 = othr & 0x1FFu, t1 = (othr >> 9) & 0x1FFu, t2 = (othr >> 18) & 0x1FFu;
    uint32_t o1 = m1 | t1, o2 = m2 | t2;
    uint32_t Tm = m2 | (~o2 & (m1 | (~o1 & m0)));  // squares whose top piece is the mover's
    uint32_t To = t2 | (~o2 & (t1 | (~o1 & t0)));  // ... the other side's
    // owner of the highest piece strictly below level k (what a lift from level k exposes)
    uint32_t um[3] = {0u, m0, m1 | (~o1 & m0)};
    uint32_t uo[3] = {0u, t0, t1 | (~o1 & t0)};
    constexpr uint32_t L[8] = {0x007u, 0x038u, 0x1C0u, 0x049u, 0x092u, 0x124u, 0x111u, 0x054u};  // board.py:135-153
    constexpr uint32_t LOW3 = 0x00100401u;   // bit 0 of each field
    constexpr uint32_t G3 = LOW3 << 9;       // guard bit of each field
    constexpr uint32_t F3 = LOW3 * 0x1FFu;   // the 9 board bits of each field
    uint32_t TmR = Tm | (Tm << 10) | (Tm << 20), ToR = To | (To << 10) | (To << 20);
    win = 0;
    lose = 0;
#pragma unroll
    for (int w = 0; w < 2; ++w) {  // word w: pieces 3w, 3w+1, 3w+2
        uint32_t lost = 0, gain = 0;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            int pi = 3 * w + f, k = pi >> 1;
            uint32_t src = ((mine & ((pi & 1) ? ~p.odd : p.odd)) >> (9 * k)) & 0x1FFu;  // where the piece stands (0: in hand)
            lost |= (src & ~um[k]) << (10 * f);  // the mover's top that leaves with the lift
            gain |= (src & uo[k]) << (10 * f);   // a piece of the other side the lift exposes
        }
        uint32_t nTm = ~(TmR & ~lost), nTo = ~(ToR | gain);  // complements of the tops after the lift
        uint32_t W = 0, Z = 0, open = F3;
#pragma unroll
        for (int l = 7; l >= 0; --l) {
            const uint32_t Lr = L[l] | (L[l] << 10) | (L[l] << 20);
            uint32_t miss = Lr & nTm;                         // squares of line l the mover lacks
            uint32_t multi = miss & ((miss | G3) - LOW3);     // != 0 in a field: two or more missing
            uint32_t mg = (multi + F3) & G3, mm = mg - (mg >> 9);
            uint32_t need = miss & ~mm;                       // destinations that complete line l
            if (!QUIET) {
                uint32_t zg = G3 & ~(miss + F3);              // fields with nothing missing: every destination
                need |= zg - (zg >> 9);
            }
            uint32_t kg = G3 & ~((Lr & nTo) + F3);            // fields where the other side holds line l
            uint32_t keep = (kg - (kg >> 9)) & ~Lr;           // ... and keeps it: destinations off the line
            uint32_t wv = need & open;
            W |= wv;
            open &= ~wv;
            uint32_t xv = keep & open;
            Z |= xv;
            open &= ~xv;
        }
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            win |= (uint64_t)((W >> (10 * f)) & 0x1FFu) << (9 * (3 * w + f));
            lose |= (uint64_t)((Z >> (10 * f)) & 0x1FFu) << (9 * (3 * w + f));
        }
    }
}

// true iff the predicate holds on ANY active lane of the wavefront (host emulation: lanes run one by one)
__device__ __forceinline__ bool wave_any(bool x)
{
#ifndef GBL_HOST_EMU
    return __any(x) != 0;
#else
    return x;
#endif
}

// outcomes54 of a ROOT position: the policy is asked about positions on which nobody holds a line (the game would be over), and
// then the QUIET form does (80 instructions less); a wavefront with a board that does hold one takes the general form.
__device__ __forceinline__ void outcomes54_root(const Planes &p, int mover, uint64_t &win, uint64_t &lose)
{
    if (wave_any(winner_of(p) != 0))
        outcomes54<false>(p, mover, win, lose);
    else
        outcomes54<true>(p, mover, win, lose);
}

// ---- the depth-2 pair evaluation's FAST form ---------------------------------------------------------------------------------
// On a position where nobody holds a line (a depth-1 result with value 0), a reply of `mover` can leave the OTHER side a
// complete line only by lifting a piece that lies directly on one of theirs, on the third square of a line they otherwise hold
// (their tops before the lift hold no line, and a lift adds exactly the square it exposes).  reply_is_plain() says that no TOP
// piece of the mover stands like that; then every line complete after a reply is the mover's, the order in which the
// reference walks the lines is irrelevant, nobody but the mover can win (`lose` = 0), and the mover's winning moves are the
// THREAT SQUARES of its tops after the lift -- squares whose two partners on some line it tops (wins54_plain: per direction
// two shifts of the tops onto the square and a mask, 12 terms, SWAR over three pieces, instead of outcomes54's eight ordered
// line steps: 119 instead of 280 instructions).  The test is conservative in one respect only: a line with two exposable squares
// counts, though one reply lifts one piece.  tests/emu checks the fast form against outcomes54 on every pair it is used for.
__device__ __forceinline__ bool reply_is_plain(const Planes &p, int mover)
{
    uint32_t mine = mover ? (p.nz & p.neg) : (p.nz & ~p.neg);
    uint32_t othr = mover ? (p.nz & ~p.neg) : (p.nz & p.neg);
    uint32_t m1 = (mine >> 9) & 0x1FFu, m2 = (mine >> 18) & 0x1FFu;
    uint32_t t0 = othr & 0x1FFu, t1 = (othr >> 9) & 0x1FFu, t2 = (othr >> 18) & 0x1FFu;
    uint32_t o1 = m1 | t1, o2 = m2 | t2;
    uint32_t To = t2 | (~o2 & (t1 | (~o1 & t0)));                    // the other side's tops
    uint32_t X = (m2 & (t1 | (~o1 & t0))) | (m1 & ~o2 & t0);         // theirs directly below a TOP piece of the mover
    uint32_t have = To | X;
    uint32_t nh = ~(have | (have << 10) | (have << 20));
    constexpr uint32_t LOW3 = 0x00100401u, G3 = LOW3 << 9, F3 = LOW3 * 0x1FFu;
    constexpr uint32_t LA = 0x007u | (0x038u << 10) | (0x1C0u << 20), LB = 0x049u | (0x092u << 10) | (0x124u << 20);
    constexpr uint32_t LC = 0x111u | (0x054u << 10) | (0x1FFu << 20);  // third field: a "line" nobody can hold
    // guard bit of a field stays clear iff none of the line's squares is missing from `have`
    uint32_t full = (G3 & ~((LA & nh) + F3)) | (G3 & ~((LB & nh) + F3)) | (G3 & ~(((LC & nh) | (1u << 20)) + F3));
    return full == 0;
}

// THREAT SQUARES, three boards at a time (10-bit fields of a word, bit 9 of each unused): the squares whose two partners on
// some line are both in T.  The partners are shifted onto the square (rows: neighbours at distance 1, columns 3, diagonal 4,
// anti-diagonal 2); the masks pick the squares for which that pair of shifts IS the line, which also keeps every term inside
// its field.
__device__ __forceinline__ uint32_t threat3(uint32_t T)
{
    constexpr uint32_t LOW3 = 0x00100401u;
    constexpr uint32_t M0 = 0x049u * LOW3, M1 = 0x092u * LOW3, M2 = 0x124u * LOW3;  // column 0 / 1 / 2 of the board, per field
    constexpr uint32_t R0 = 0x007u * LOW3, R1 = 0x038u * LOW3, R2 = 0x1C0u * LOW3;  // row 0 / 1 / 2
    constexpr uint32_t B0 = 0x001u * LOW3, B2 = 0x004u * LOW3, B4 = 0x010u * LOW3, B6 = 0x040u * LOW3, B8 = 0x100u * LOW3;
    return ((T >> 1) & (T >> 2) & M0) | ((T << 1) & (T >> 1) & M1) | ((T << 1) & (T << 2) & M2)    // (0,1,2) (3,4,5) (6,7,8)
         | ((T >> 3) & (T >> 6) & R0) | ((T << 3) & (T >> 3) & R1) | ((T << 3) & (T << 6) & R2)    // (0,3,6) (1,4,7) (2,5,8)
         | ((T >> 4) & (T >> 8) & B0) | ((T << 4) & (T >> 4) & B4) | ((T << 4) & (T << 8) & B8)    // (0,4,8)
         | ((T >> 2) & (T >> 4) & B2) | ((T << 2) & (T >> 2) & B4) | ((T << 2) & (T << 4) & B6);   // (2,4,6)
}

// the mover's winning moves on a quiet position whose replies are plain (see above); bit a as in outcomes54's `win`
__device__ __forceinline__ uint64_t wins54_plain(const Planes &p, int mover)
{
    uint32_t mine = mover ? (p.nz & p.neg) : (p.nz & ~p.neg);
    uint32_t othr = mover ? (p.nz & ~p.neg) : (p.nz & p.neg);
    uint32_t m0 = mine & 0x1FFu, m1 = (mine >> 9) & 0x1FFu, m2 = (mine >> 18) & 0x1FFu;
    uint32_t t1 = (othr >> 9) & 0x1FFu, t2 = (othr >> 18) & 0x1FFu;
    uint32_t o1 = m1 | t1, o2 = m2 | t2;
    uint32_t Tm = m2 | (~o2 & (m1 | (~o1 & m0)));  // squares whose top piece is the mover's
    uint32_t um[3] = {0u, m0, m1 | (~o1 & m0)};    // the mover's highest piece strictly below level k
    uint32_t TmR = Tm | (Tm << 10) | (Tm << 20);
    uint64_t win = 0;
#pragma unroll
    for (int w = 0; w < 2; ++w) {  // word w: pieces 3w, 3w+1, 3w+2 in 10-bit fields
        uint32_t lost = 0;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            int pi = 3 * w + f, k = pi >> 1;
            uint32_t src = ((mine & ((pi & 1) ? ~p.odd : p.odd)) >> (9 * k)) & 0x1FFu;  // where the piece stands (0: in hand)
            lost |= (src & ~um[k]) << (10 * f);  // the mover's top that leaves with the lift
        }
        const uint32_t W = threat3(TmR & ~lost);
#pragma unroll
        for (int f = 0; f < 3; ++f) win |= (uint64_t)((W >> (10 * f)) & 0x1FFu) << (9 * (3 * w + f));
    }
    return win;
}

// reply_is_plain(moved(p, me, a), 1 - me) for ALL moves a of `me` at once: bit a SET = NOT plain, the pair (p, a) takes the
// ordered form of the evaluation.  With H = our tops and the squares where a TOP piece of the opponent lies directly on one of
// ours -- the set reply_is_plain looks for a full line in -- a move of our piece i from s (nowhere: in hand) to q changes H in
// two squares only: q joins it (our piece is the top there now, whatever lay there), and s stays iff what the lift leaves on
// top of s is ours, or the opponent's lying directly on a piece of ours (the set C below); every other stack is as it was.
// So per piece B_i = (H - s) + (C & s), and the pair is not plain iff B_i + q holds a full line: iff B_i does already, or q is
// a threat square of B_i -- the threat squares of six 9-bit sets in two words.  One wavefront that idles through the depth-1
// walk does this for a whole tile; the work lists are then split by it.  tests/emu checks every candidate's bit against
// reply_is_plain on the moved board.
__device__ __forceinline__ uint64_t greedy_nonplain(const Planes &p, int me)
{
    const uint32_t mine = me ? (p.nz & p.neg) : (p.nz & ~p.neg);
    const uint32_t othr = me ? (p.nz & ~p.neg) : (p.nz & p.neg);
    const uint32_t m0 = mine & 0x1FFu, m1 = (mine >> 9) & 0x1FFu, m2 = (mine >> 18) & 0x1FFu;
    const uint32_t t0 = othr & 0x1FFu, t1 = (othr >> 9) & 0x1FFu, t2 = (othr >> 18) & 0x1FFu;
    const uint32_t o1 = m1 | t1, o2 = m2 | t2;
    const uint32_t below2 = m1 | (~o1 & m0);                      // our piece is the highest one strictly below level 2
    const uint32_t Tm = m2 | (~o2 & below2);                      // our tops
    const uint32_t X = (t2 & below2) | (t1 & ~o2 & m0);           // ours directly below a TOP piece of the opponent
    const uint32_t H = Tm | X;
    const uint32_t C = (m2 & (below2 | (t1 & m0))) | (m1 & ~o2 & m0);  // squares of H that stay when our top piece leaves
    const uint32_t HR = H | (H << 10) | (H << 20), CR = C | (C << 10) | (C << 20);
    constexpr uint32_t LOW3 = 0x00100401u, G3 = LOW3 << 9, F3 = LOW3 * 0x1FFu;
    uint64_t np = 0;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        uint32_t src = 0;
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            const int pi = 3 * w + f, k = pi >> 1;
            src |= (((mine & ((pi & 1) ? ~p.odd : p.odd)) >> (9 * k)) & 0x1FFu) << (10 * f);  // where the piece stands
        }
        const uint32_t B = (HR & ~src) | (CR & src);
        const uint32_t th = threat3(B);
        const uint32_t fg = (((th & B) + F3) & G3);  // a full line inside B itself: guard bit of the field
        const uint32_t N = th | (fg - (fg >> 9));
#pragma unroll
        for (int f = 0; f < 3; ++f) np |= (uint64_t)((N >> (10 * f)) & 0x1FFu) << (9 * (3 * w + f));
    }
    return np;
}

__device__ __forceinline__ uint64_t below_eq(int b) { return (2ull << b) - 1ull; }  // bits 0..b, b < 63

// One decision for the agent `me` on board p, in four per-board pieces so that a kernel can spread
// the expensive one (greedy_reply) over the lanes of a wavefront.  `mask` is the legal mask handed to
// the policy (greedy_policy.py:76), prev3 the agent's last three actions packed one per byte (0xFF =
// none).  The reference's control flow -- the depth-1 loop (:84-101), the depth-2 loop with its
// order-dependent pruning (:103-157), the fallback test (:211-214) -- is replayed in order over
// outcome bit-sets, so that no per-leaf loop remains: per depth-1 candidate one moved(), one
// legal54() and one outcomes54() give every opponent reply's result.
struct GreedyHead {
    uint64_t cands;     // actions_depth1 as a 54-bit set, :77-79
    uint64_t todo;      // depth-1 results with value 0, in insertion (= ascending) order: the depth-2 loop's list
    uint64_t legal_me;  // board.is_legal(agent_index, a) on the root position, :85 and :141
    uint64_t dup;       // candidates in todo whose reply summary equals that of candidate a - 9 (see greedy_head)
    int ncands, chosen;
};

// depth 1, :84-101
__device__ __forceinline__ GreedyHead greedy_head(const Planes &p, int me, uint64_t mask, int depth)
{
    GreedyHead h;
    h.cands = mask;
    h.ncands = __popcll(mask);
    h.chosen = -1;
    h.legal_me = legal54(p, me);
    uint64_t tried = mask & h.legal_me;  // actions the depth-1 loop evaluates, ascending
    uint64_t win1, lose1;
    outcomes54_root(p, me, win1, lose1);
    win1 &= tried;
    lose1 &= tried;
    // The walk over the decisive results in order (:92-101), in CLOSED FORM (round 5: the loop ran as long as the busiest lane's
    // count of decisive moves, on the owners' path of the greedy kernels' B phase).  Let fw be the first winning move.  Every
    // losing move before it takes itself off actions_depth1 while more than one action is left (:95-99) -- and since the losing
    // moves are candidates themselves, the list can only run down to one if EVERY candidate loses (no win before the last one):
    // then the walk stops at the last of them (:100-101) with that one left.  Otherwise all losing moves before fw go, and the
    // walk ends at fw (chosen, :92-94) or runs through.  Everything before the stop is in `results`.
    const uint64_t before_fw = win1 ? (1ull << __builtin_ctzll(win1)) - 1ull : ~0ull;
    const uint64_t lb = lose1 & before_fw;                    // the losing moves the walk meets
    const int m = __popcll(lb);
    const bool all_lose = m > 0 && m == h.ncands;             // (then there is no win among the tried moves either)
    const int last = all_lose ? 63 - __builtin_clzll(lb) : 0;
    h.cands = all_lose ? (1ull << last) : (h.cands & ~lb);
    h.ncands = all_lose ? 1 : h.ncands - m;
    h.chosen = win1 ? __builtin_ctzll(win1) : -1;
    uint64_t seen = win1 ? (tried & (before_fw | (before_fw + 1ull))) : all_lose ? (tried & below_eq(last)) : tried;
    // :103; depth 3 adds :160-208, whose only assignment repeats :157 -- no effect
    h.todo = depth > 1 ? (seen & ~win1 & ~lose1) : 0ull;
    // The two pieces of a size are interchangeable: while both are still in hand, placing piece 2k+1 on q
    // gives the opponent exactly the position that placing piece 2k there does (the planes differ in one
    // `odd` bit of OUR piece, which none of the opponent's legality / outcome terms reads), so candidate
    // a + 9 has the reply summary of candidate a.  27 % of the candidates on the masked-random mix.
    uint32_t mine = me ? (p.nz & p.neg) : (p.nz & ~p.neg);
    h.dup = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint64_t both = (h.todo >> (18 * k)) & (h.todo >> (18 * k + 9)) & 0x1FFull;
        if (((mine >> (9 * k)) & 0x1FFu) == 0) h.dup |= both << (18 * k + 9);
    }
    return h;
}

// all placements of `me`'s pieces that are still in hand (54-bit set)
__device__ __forceinline__ uint64_t greedy_from_hand(const Planes &p, int me)
{
    const uint32_t mine = me ? (p.nz & p.neg) : (p.nz & ~p.neg);
    uint64_t from_hand = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t lvl = (mine >> (9 * k)) & 0x1FFu, oddp = (p.odd >> (9 * k)) & 0x1FFu;
        if ((lvl & oddp) == 0) from_hand |= 0x1FFull << (18 * k);        // piece 2k
        if ((lvl & ~oddp) == 0) from_hand |= 0x1FFull << (18 * k + 9);   // piece 2k + 1
    }
    return from_hand;
}

// have = a 9-bit set of squares: the squares that complete a line inside it (exactly one square of the line missing) -- or every
// square, if it holds a complete line already.  As threat squares (round 4: ~35 instead of the eight-line walk's ~60 instructions, on
// the longest wavefront of the greedy kernels' B phase): a square both of whose partners on some line are in `have` is a threat
// square; one that is itself in `have` means a full line.  tests/emu checks all 512 sets against the line walk.
__device__ __forceinline__ uint32_t risky_from_have(uint32_t have)
{
    const uint32_t th = threat3(have & 0x1FFu) & 0x1FFu;  // (one field; what the shifts push into the fields above is masked off)
    return (th & have) ? 0x1FFu : th;
}

// The squares on which a placement of ours could let a LIFT by the opponent hand us a line (then the opponent's replies
// are not just "the root's winning moves, minus the defused ones", see below): with "have" = our tops and our pieces
// directly under the opponent's, the squares that complete a line inside have -- or every square, if have holds a line already.
__device__ __forceinline__ uint32_t greedy_risky_squares(const Planes &p, int me)
{
    const uint32_t mine = me ? (p.nz & p.neg) : (p.nz & ~p.neg);
    const uint32_t othr = me ? (p.nz & ~p.neg) : (p.nz & p.neg);
    const uint32_t t0 = mine & 0x1FFu, t1 = (mine >> 9) & 0x1FFu, t2 = (mine >> 18) & 0x1FFu;
    const uint32_t m1 = (othr >> 9) & 0x1FFu, m2 = (othr >> 18) & 0x1FFu;
    const uint32_t o1 = m1 | t1, o2 = m2 | t2;
    const uint32_t To = t2 | (~o2 & (t1 | (~o1 & t0)));       // our tops
    const uint32_t X = (m1 & t0) | (m2 & (t1 | (~o1 & t0)));  // ours directly below a piece of the opponent's
    return risky_from_have((To | X) & 0x1FFu);
}

// ---- placements from hand, settled from the ROOT position alone (round 3) ------------------------------------------------
// Let R be the OPPONENT's winning moves on the root, were it to move.  After a placement `a` of ours from hand on q every
// winning reply is in R: a reply that wins after `a` is legal on the root too (we only covered q) and finds there the same
// tops except that q is what it was instead of ours -- which only helps the opponent -- or, if it gobbles our new piece,
// exactly the same tops.  And a2 = (piece pj, square q2) in R stops winning ("is defused") exactly if
//   q is where pj stands (we gobbled it: it cannot move), or
//   q = q2 and our piece is at least as large as pj (the reply is no longer legal), or
//   q != q2 lies on EVERY line the opponent holds after a2 (each of them now has our piece on it),
// provided no lift by the opponent can hand US a line, which with "have" = our tops and our pieces directly under the
// opponent's is the case iff q does not complete a line inside have (greedy_risky_squares).  So for the
// placements from hand on non-risky squares the whole summary -- first / second winning reply, the first one we could
// play ourselves -- follows from R and a few set operations per member of R, with no depth-2 evaluation at all: two
// thirds of the (board, candidate) pairs of the masked-random mix.  Placements on risky squares are evaluated.  (R empty
// -- half of the boards -- means: none of these placements has a winning reply.)  Pinned against the exact evaluation on every candidate it settles: tests/emu (emu_greedy_root_rule).
struct GreedyRoot {
    uint64_t replies;    // R: the opponent's winning moves on the root
    uint32_t risky;      // 9 bits: squares where a placement of ours is not "plain" (0x1FF if have already holds a line)
};

__device__ __forceinline__ uint64_t spread9(uint32_t squares)  // a 9-bit set of squares under all six pieces
{
    uint64_t x = squares & 0x1FFu;
    x |= x << 9;
    return x | x << 18 | x << 36;
}

__device__ __forceinline__ GreedyRoot greedy_root(const Planes &p, int me)
{
    uint64_t ow, ol;
    outcomes54_root(p, 1 - me, ow, ol);  // (the root itself need not be free of lines)
    return GreedyRoot{ow & legal54(p, 1 - me), greedy_risky_squares(p, me)};
}

// the placements from hand (of any of our pieces, on any square: mask with the candidates) that do NOT defuse the
// opponent's winning move a2 of the root
__device__ __forceinline__ uint64_t greedy_undefused(const Planes &p, int me, uint32_t a2)
{
    const int opp = 1 - me;
    const uint32_t pj = (a2 * 57u) >> 9, q2 = a2 - 9u * pj, kj = pj >> 1, first = (~pj) & 1u;
    const uint32_t theirs = me ? (p.nz & ~p.neg) : (p.nz & p.neg);
    const uint32_t stands = ((theirs & (first ? p.odd : ~p.odd)) >> (9u * kj)) & 0x1FFu;  // where pj stands (0: in hand)
    const Planes d = moved(p, opp, a2);
    const uint32_t ours_d = me ? (d.nz & d.neg) : (d.nz & ~d.neg), theirs_d = me ? (d.nz & ~d.neg) : (d.nz & d.neg);
    const uint32_t t0 = theirs_d & 0x1FFu, t1 = (theirs_d >> 9) & 0x1FFu, t2 = (theirs_d >> 18) & 0x1FFu;
    const uint32_t m1 = (ours_d >> 9) & 0x1FFu, m2 = (ours_d >> 18) & 0x1FFu;
    const uint32_t o1 = m1 | t1, o2 = m2 | t2;
    const uint32_t Tt = t2 | (~o2 & (t1 | (~o1 & t0)));  // the opponent's tops after a2
    constexpr uint32_t L[8] = {0x007u, 0x038u, 0x1C0u, 0x049u, 0x092u, 0x124u, 0x111u, 0x054u};
    uint32_t every = 0x1FFu;  // squares on every line the opponent then holds
#pragma unroll
    for (int l = 0; l < 8; ++l) every &= (L[l] & ~Tt) == 0 ? L[l] : 0x1FFu;
    const uint32_t q2bit = 1u << q2, defuse = stands | (every & ~q2bit);
    uint64_t u = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
        const uint64_t uk = ~(defuse | (k >= kj ? q2bit : 0u)) & 0x1FFu;
        u |= uk << (18u * k) | uk << (18u * k + 9u);
    }
    return u;
}

// The rule in the shape the kernel uses it: the members of R are dealt out as ITEMS (board, j), j = the member's rank in
// R, to whichever lane is free; an item's lane leaves undef[j] = greedy_undefused(R's j-th member) & resolved in the
// board's table, and the board's owner merges the table in ascending order -- the reference's reply order -- into the
// candidate sets of greedy_replay_closed.  Boards with more than kRootItems members (rare) do not use the rule.
constexpr int kRootItems = 6;

struct GreedyHandSets {
    uint64_t threat, second, block, flegal;
};

__device__ __forceinline__ GreedyHandSets greedy_hand_merge(uint64_t replies, uint64_t legal_me, const uint64_t (&undef)[kRootItems])
{
    GreedyHandSets s{0ull, 0ull, 0ull, 0ull};
    uint64_t it = replies;
#pragma unroll
    for (int j = 0; j < kRootItems; ++j) {
        const bool live = it != 0;
        const uint32_t a2 = live ? (uint32_t)__builtin_ctzll(it) : 0u;
        const uint64_t u = live ? undef[j] : 0ull;
        const bool ours = live && ((legal_me >> a2) & 1ull);
        s.second |= u & s.threat;
        s.flegal |= ours ? (u & ~s.threat) : 0ull;  // the FIRST winning reply is a legal move of ours
        s.block |= ours ? u : 0ull;
        s.threat |= u;
        it &= it - 1;
    }
    return s;
}

// the 16-bit summary (see greedy_reply) of ONE settled placement `a`, from the board's table
__device__ __forceinline__ uint32_t greedy_hand_lookup(uint64_t replies, uint64_t legal_me, const uint64_t (&undef)[kRootItems], uint32_t a)
{
    uint64_t ow = 0, it = replies;
#pragma unroll
    for (int j = 0; j < kRootItems; ++j) {
        const bool live = it != 0;
        const uint32_t a2 = live ? (uint32_t)__builtin_ctzll(it) : 0u;
        if (live && ((undef[j] >> a) & 1ull)) ow |= 1ull << a2;
        it &= it - 1;
    }
    const uint64_t block = ow & legal_me;
    uint32_t s = ow ? 1u : 0u;
    s |= (ow ? (uint32_t)__builtin_ctzll(ow) : 0u) << 1;
    s |= (ow & (ow - 1)) ? 1u << 7 : 0u;
    s |= block ? 1u << 8 : 0u;
    s |= (block ? (uint32_t)__builtin_ctzll(block) : 0u) << 9;
    return s;
}

// The same two in the form the kernel's owners run them (round 4): an item's lane TAGS its table row -- bits 0-53 the set
// greedy_undefused gives, bits 56-61 the member a2 itself, bit 63 "a2 is a legal move of ours on the root" -- so that the owner's
// merge needs neither the k-th member of R (a 64-bit find-first-set and clear per step) nor a 64-bit shift of its legal set:
// the rows are in rank order, row j is live iff j < |R|, and everything else is in the row.  ~14 instead of ~30 instructions per
// step of a loop that runs on ONE wavefront per SIMD.  tests/emu runs the kernel's walk through these and checks every settled
// candidate against the exact evaluation, as before.
__device__ __forceinline__ uint64_t greedy_item_row(const Planes &p, int me, uint64_t legal_me, uint32_t a2)
{
    return greedy_undefused(p, me, a2) | ((uint64_t)a2 << 56) | (((legal_me >> a2) & 1ull) << 63);
}

__device__ __forceinline__ GreedyHandSets greedy_hand_merge_tagged(int n, uint64_t resolved, const uint64_t (&rows)[kRootItems])
{
    GreedyHandSets s{0ull, 0ull, 0ull, 0ull};
#pragma unroll
    for (int j = 0; j < kRootItems; ++j) {
        const bool live = j < n;
        const uint64_t u = live ? rows[j] & resolved : 0ull;     // (resolved has no bit above 53: the tags go with the mask)
        const bool ours = live && (int64_t)rows[j] < 0;
        s.second |= u & s.threat;
        s.flegal |= ours ? (u & ~s.threat) : 0ull;  // the FIRST winning reply is a legal move of ours
        s.block |= ours ? u : 0ull;
        s.threat |= u;
    }
    return s;
}

__device__ __forceinline__ uint32_t greedy_hand_lookup_tagged(int n, uint64_t legal_me, const uint64_t (&rows)[kRootItems], uint32_t a)
{
    uint64_t ow = 0;
#pragma unroll
    for (int j = 0; j < kRootItems; ++j)
        if (j < n && ((rows[j] >> a) & 1ull)) ow |= 1ull << ((uint32_t)(rows[j] >> 56) & 63u);
    const uint64_t block = ow & legal_me;
    uint32_t s = ow ? 1u : 0u;
    s |= (ow ? (uint32_t)__builtin_ctzll(ow) : 0u) << 1;
    s |= (ow & (ow - 1)) ? 1u << 7 : 0u;
    s |= block ? 1u << 8 : 0u;
    s |= (block ? (uint32_t)__builtin_ctzll(block) : 0u) << 9;
    return s;
}

// Which candidates are evaluated (exactly, in the pooled round), which are settled from the root, and the root's
// replies if they are to be dealt out as items.
struct GreedyRootPlan {
    uint64_t eval, resolved, items;
};

__device__ __forceinline__ GreedyRootPlan greedy_root_plan(const GreedyHead &h, const Planes &p, int me, const GreedyRoot &g)
{
    const uint64_t w0 = h.todo & ~h.dup;
    const bool rule = __popcll(g.replies) <= kRootItems;
    const uint64_t resolved = rule ? (w0 & greedy_from_hand(p, me) & ~spread9(g.risky)) : 0ull;
    return GreedyRootPlan{w0 & ~resolved, resolved, resolved ? g.replies : 0ull};
}

// What the depth-2 loop needs to know about candidate `a` (:107-126), packed in 16 bits:
//   bit 0      the opponent has a winning reply            (ow != 0)
//   bits 1-6   the first winning reply f
//   bit 7      there is a second one
//   bit 8      some winning reply is a legal move of ours on the root position (:141)
//   bits 9-14  the first such reply
//   bit 15     every reply wins the game for us            (all(), :146-149; implies bit 0 clear)
// PLAIN: the caller has checked greedy_pair_is_plain(p, me, a) -- the fast form (threat squares; nobody but the opponent
// can win, so "every reply wins for us" holds only if the opponent cannot move at all); otherwise outcomes54's ordered line steps.
__device__ __forceinline__ bool greedy_pair_is_plain(const Planes &p, int me, uint32_t a)
{
    return reply_is_plain(moved(p, me, a), 1 - me);
}

template <bool PLAIN = false>
__device__ __forceinline__ uint32_t greedy_reply(const Planes &p, int me, uint64_t legal_me, uint32_t a)
{
    const int opp = 1 - me;
    Planes d1 = moved(p, me, a);         // :107-109
    uint64_t legal2 = legal54(d1, opp);  // :112-116
    uint64_t ow, mw;                     // the opponent wins / we win after reply a2, :120-126
    if (PLAIN) {
        ow = wins54_plain(d1, opp);
        mw = 0;
    } else {
        outcomes54<true>(d1, opp, ow, mw);  // (a is a depth-1 result with value 0: nobody holds a line on d1)
    }
    ow &= legal2;
    mw &= legal2;
    uint64_t block = ow & legal_me;
    uint32_t s = ow ? 1u : 0u;
    s |= (ow ? (uint32_t)__builtin_ctzll(ow) : 0u) << 1;
    s |= (ow & (ow - 1)) ? 1u << 7 : 0u;
    s |= block ? 1u << 8 : 0u;
    s |= (block ? (uint32_t)__builtin_ctzll(block) : 0u) << 9;
    s |= (legal2 & ~mw) == 0 ? 1u << 15 : 0u;
    return s;
}

// :129-143 for a candidate a whose summary s has bit 0 set.  none_yet: `chosen_action is None` (:142) can
// still hold as far as the candidates WITHOUT a winning reply are concerned (h.chosen tracks the rest).
__device__ __forceinline__ void greedy_threat(GreedyHead &h, int a, uint32_t s, bool none_yet)
{
    int f = (int)((s >> 1) & 63u);
    if (h.ncands > 1) {
        if ((h.cands >> a) & 1ull) {
            h.cands &= ~(1ull << a);
            --h.ncands;
        }
        if (h.ncands > 1 || !(s & (1u << 7))) {  // no break: every opponent win is looked at
            if (none_yet && h.chosen < 0 && (s & (1u << 8))) h.chosen = (int)((s >> 9) & 63u);
        } else {                                  // break at the second opponent win
            if (none_yet && h.chosen < 0 && ((h.legal_me >> f) & 1ull)) h.chosen = f;
        }
    }                                             // else: break at the first opponent win
}

// One iteration of the depth-2 loop (:129-157) for candidate a with summary s; true = `break` (:151).
// With a winning reply f among the evaluated replies neither all() can hold (f is evaluated in
// every early-break variant), so only the no-winning-reply case reaches :146-157.
__device__ __forceinline__ bool greedy_replay(GreedyHead &h, int a, uint32_t s)
{
    if (s & 1u) {
        greedy_threat(h, a, s, true);
        return false;
    }
    h.chosen = a;              // all(... != their win), :153-157 -- or all(... == our win), :146-151
    return (s >> 15) & 1u;
}

// The whole depth-2 loop from two candidate sets -- threat: summaries with bit 0, allwin: with bit 15 --
// looking up summaries only for the (few) candidates in `threat`.  A candidate without a winning reply
// assigns chosen_action unconditionally (:157, :150), so the last of them before the :151 break is
// the result if there is one, and from the first of them on `chosen_action is None` (:142) is false.
template <typename ReplyOf>
__device__ __forceinline__ void greedy_replay_sets(GreedyHead &h, uint64_t threat, uint64_t allwin, ReplyOf reply_of)
{
    uint64_t todo = h.todo;
    threat |= (threat << 9) & h.dup;  // twin placements share their partner's summary (reply_of must serve them too)
    allwin |= (allwin << 9) & h.dup;
    allwin &= todo;
    if (allwin) todo &= below_eq(__builtin_ctzll(allwin));  // :151: nothing after the break is looked at
    const uint64_t calm = todo & ~threat;
    const uint64_t before_calm = calm ? (1ull << __builtin_ctzll(calm)) - 1ull : ~0ull;
    for (uint64_t it = threat & todo; it; it &= it - 1) {
        const int a = __builtin_ctzll(it);
        greedy_threat(h, a, reply_of(a), (before_calm >> a) & 1ull);
    }
    if (calm) h.chosen = 63 - __builtin_clzll(calm);
}

// position of the k-th (0-based) set bit of a 54-bit set; k < popcount(m)
__device__ __forceinline__ uint32_t kth_bit64(uint64_t m, uint32_t k)
{
    const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32), nlo = __popc(lo);
    const bool low = k < nlo;
    return kth_bit32(low ? lo : hi, low ? k : k - nlo) + (low ? 0u : 32u);
}

// The depth-2 loop (:103-157) in CLOSED FORM -- no per-candidate iteration.  What the loop does with a candidate
// that has a winning reply (greedy_threat) depends on the candidate only through three bits of its summary and on
// how many such candidates came before it:
//   * each of them takes itself off actions_depth1 while more than one action is left (:129-134), so the j-th of
//     them (j = 0, 1, ...) is handled iff j < n0 - 1 (n0 = len(actions_depth1) on entry), and those removed are the
//     first min(count, n0 - 1) of the set;
//   * the reply loop breaks at the SECOND opponent win only when the removal left a single action (:135-143), i.e.
//     for j = n0 - 2 only; every earlier one looks at all opponent wins and proposes the first that we could play
//     ourselves (summary bit 8), the one at j = n0 - 2 with a second winning reply (bit 7) proposes the FIRST winning
//     reply if that is a legal move of ours;
//   * a proposal is taken only while chosen_action is None (:142): before the first candidate without a winning
//     reply, and only the first proposal counts.
// So the loop's effect is a handful of set operations on per-board candidate sets, which the evaluating lanes
// accumulate: threat (summary bit 0), allwin (bit 15), second (bit 7), block (bit 8), flegal (first winning reply is
// a legal move of ours) -- plus ONE summary lookup, for the candidate whose proposal is taken.
struct ReplySets {
    uint64_t threat, allwin, second, block, flegal;
};

template <typename ReplyOf>
__device__ __forceinline__ void greedy_replay_closed(GreedyHead &h, ReplySets r, ReplyOf reply_of)
{
    uint64_t todo = h.todo;
    // twin placements share their partner's summary (reply_of must serve them too)
    r.threat |= (r.threat << 9) & h.dup;
    r.allwin |= (r.allwin << 9) & h.dup;
    r.second |= (r.second << 9) & h.dup;
    r.block |= (r.block << 9) & h.dup;
    r.flegal |= (r.flegal << 9) & h.dup;
    r.allwin &= todo;
    if (r.allwin) todo &= below_eq(__builtin_ctzll(r.allwin));  // :151: nothing after the break is looked at
    const uint64_t calm = todo & ~r.threat;
    const uint64_t before_calm = calm ? (1ull << __builtin_ctzll(calm)) - 1ull : ~0ull;
    const uint64_t th = r.threat & todo & h.cands;  // (every candidate of todo is still in actions_depth1)
    const int m = __popcll(th), n0 = h.ncands;
    if (m > 0 && n0 > 1) {
        // A: the first n0 - 2 of th (they never break early); e: the one after them, if any
        uint64_t A = th, e = 0;
        if (n0 - 2 < m) {
            e = 1ull << kth_bit64(th, (uint32_t)(n0 - 2));
            A = th & (e - 1ull);
        }
        const uint64_t e_prop = (e & r.second) ? (e & r.flegal) : (e & r.block);
        const uint64_t prop = before_calm & ((A & r.block) | e_prop);
        if (h.chosen < 0 && prop) {
            const int a = __builtin_ctzll(prop);
            const uint32_t s = reply_of(a);
            const bool early = ((e >> a) & 1ull) && ((r.second >> a) & 1ull);  // broke at the second opponent win
            h.chosen = early ? (int)((s >> 1) & 63u) : (int)((s >> 9) & 63u);
        }
        const uint64_t removed = A | e;
        h.cands &= ~removed;
        h.ncands = n0 - __popcll(removed);
    }
    if (calm) h.chosen = 63 - __builtin_clzll(calm);
}

// :211-214
__device__ __forceinline__ GreedyResult greedy_finish(const GreedyHead &h, uint32_t prev3)
{
    uint32_t c = (uint32_t)h.chosen;
    bool fb = h.chosen < 0 || (prev3 & 0xFFu) == c || ((prev3 >> 8) & 0xFFu) == c || ((prev3 >> 16) & 0xFFu) == c;
    return GreedyResult{h.chosen, h.cands, fb};
}

// the four pieces in sequence on one board
__device__ __forceinline__ GreedyResult greedy_decide(const Planes &p, int me, uint64_t mask, int depth, uint32_t prev3)
{
    GreedyHead h = greedy_head(p, me, mask, depth);
    for (uint64_t it = h.todo; it;) {
        int a = __builtin_ctzll(it);
        it &= it - 1;
        const uint32_t twin = ((h.dup >> a) & 1ull) ? (uint32_t)a - 9u : (uint32_t)a;  // same summary, see greedy_head
        if (greedy_replay(h, a, greedy_reply(p, me, h.legal_me, twin))) break;
    }
    return greedy_finish(h, prev3);
}

// ---- gbl_tree_search: leaf-parallel UCT, one tree per board (contract: include/gobblet_hip.h) --
// Integer-only, so that k_tree, the host flavour and a restatement of the contract agree bit for bit.  The tree is an array of
// 16-byte nodes (LDS in the kernel, a vector in the host flavour); node 0 is the root, 0 in a link stands for "none".  A node
// holds no position: selection replays the actions from the root planes, one move_planes per level.
constexpr uint32_t kStreamTree = 3u;  // generator stream of the search: the expansion draws and the leaves' playouts
constexpr int kTreeMaxIterations = 1024, kTreeMaxPlayouts = 256, kTreeMaxExplore = 1024;
// what the move INTO a node decided: nothing, a win / a loss of the side that made it, or a side to move without a legal action
constexpr uint32_t kTreeOpen = 0u, kTreeWon = 1u, kTreeLost = 2u, kTreeStuck = 3u;

struct TreeNode {
    uint16_t parent, child, sibling, n;  // links (child = the newest child, sibling = the next older one); n <= 1024 visits
    uint32_t w, l;                       // W | action << 24,  L | kTree* << 24   (W, L <= 1024 * 256 = 2^18)
};
static_assert(sizeof(TreeNode) == 16, "a tree node is 16 bytes");

__device__ __forceinline__ uint32_t tree_action(const TreeNode &v) { return v.w >> 24; }
__device__ __forceinline__ uint32_t tree_term(const TreeNode &v) { return v.l >> 24; }
__device__ __forceinline__ uint32_t tree_wins(const TreeNode &v) { return v.w & 0xFFFFFFu; }
__device__ __forceinline__ uint32_t tree_losses(const TreeNode &v) { return v.l & 0xFFFFFFu; }

// generator id of playout j of iteration i of global board g (j = 0, word 0: the expansion draw).  Independent of the number of
// iterations and of playouts: a longer search is a continuation of a shorter one.
__device__ __forceinline__ uint64_t tree_pid(uint64_t g, uint32_t i, uint32_t j) { return (g * 1024ull + i) * 256ull + j; }

// exact integer square root of x < 2^24
__device__ __forceinline__ uint32_t tree_isqrt(uint32_t x)
{
    uint32_t r = 0;
#pragma unroll
    for (uint32_t b = 1u << 22; b; b >>= 2) {
        const bool ge = x >= r + b;
        x -= ge ? r + b : 0u;
        r = (r >> 1) + (ge ? b : 0u);
    }
    return r;
}

// The selection key of a child (n visits, W wins, L losses of the side choosing) under a parent of np visits:
//   ((W - L + n P) << 15) / (n P)  +  ((explore * isqrt((bitlen(np) << 20) / n)) >> 3)
// The first quotient is taken in two base-2^8 steps of long division, which keeps every operand below 2^32 (W - L + n P <= 2^19).
__device__ __forceinline__ uint32_t tree_key(uint32_t W, uint32_t L, uint32_t n, uint32_t P, uint32_t np, uint32_t explore)
{
    const uint32_t d = n * P, x = W + d - L;
    const uint32_t hi = (x << 7) / d, rem = (x << 7) - hi * d;
    const uint32_t mean = (hi << 8) + (rem << 8) / d;
    const uint32_t bitlen = np ? 32u - (uint32_t)__builtin_clz(np) : 0u;
    return mean + ((explore * tree_isqrt((bitlen << 20) / n)) >> 3);
}
// the order of the children of one node: the larger key, then the lower action (key < 2^20); 0 stands for "no child"
__device__ __forceinline__ uint32_t tree_order_key(uint32_t key, uint32_t a) { return ((key + 1u) << 6) | (63u - a); }
// the order of the root's children for the decision: visits, then W - L, then the lower action; 0 stands for "no child"
__device__ __forceinline__ uint64_t tree_final_key(uint32_t n, uint32_t W, uint32_t L, uint32_t a)
{
    return ((uint64_t)n << 32) | (uint64_t)(((W + (1u << 18) - L) << 6) | (63u - a));
}
__device__ __forceinline__ int tree_action_of(uint64_t best_key) { return best_key ? 63 - (int)(best_key & 63u) : -1; }

// Where an iteration's selection stopped: at `node`, whose position is p with `side` to move.  untried = its candidates without
// a child (non-empty: the iteration expands one of them); 0: the node is terminal and is evaluated itself.
struct TreeLeaf {
    uint32_t node;
    Planes p;
    int side;
    uint64_t untried;
};

// Step 1, one node after the other (the host flavour; k_tree walks the same rule with a lane per child).  rootcand != 0.
__device__ __forceinline__ TreeLeaf tree_select(const TreeNode *nodes, const Planes &root, int mover, uint64_t rootcand, uint32_t P,
                                                uint32_t explore)
{
    TreeLeaf s{0u, root, mover, 0ull};
    uint64_t cand = rootcand;
    for (;;) {
        const TreeNode v = nodes[s.node];
        if (tree_term(v)) return s;
        uint64_t have = 0;
        uint32_t best = 0, best_c = 0;
        for (uint32_t c = v.child; c; c = nodes[c].sibling) {
            const TreeNode k = nodes[c];
            have |= 1ull << tree_action(k);
            const uint32_t key = tree_order_key(tree_key(tree_wins(k), tree_losses(k), k.n, P, v.n, explore), tree_action(k));
            if (key > best) best = key, best_c = c;
        }
        s.untried = cand & ~have;
        if (s.untried) return s;
        move_planes(s.p, s.side, tree_action(nodes[best_c]));
        s.side ^= 1;
        s.node = best_c;
        cand = legal54(s.p, s.side);
    }
}

// Step 2 without the bookkeeping: the gbl_sample rule over the untried candidates on generator word r, the move, and what it
// decided (kTree*).  p / side become the new child's position.  Returns the action.
__device__ __forceinline__ uint32_t tree_move_into(Planes &p, int &side, uint32_t a)  // the move, and what it decided (kTree*)
{
    const int by = side;
    move_planes(p, side, a);
    side ^= 1;
    const int w = winner_of(p);
    const int mine = by ? -w : w;
    return mine > 0 ? kTreeWon : (mine < 0 ? kTreeLost : (legal54(p, side) ? kTreeOpen : kTreeStuck));
}

__device__ __forceinline__ uint32_t tree_expand_move(Planes &p, int &side, uint64_t untried, uint32_t r, uint32_t &term)
{
    const uint32_t a = kth_bit64(untried, __umulhi(r, (uint32_t)__popcll(untried)));
    term = tree_move_into(p, side, a);
    return a;
}

// ... and the bookkeeping: node `at` becomes the newest child of `parent`
__device__ __forceinline__ void tree_link(TreeNode *nodes, uint32_t at, uint32_t parent, uint32_t a, uint32_t term)
{
    nodes[at] = TreeNode{(uint16_t)parent, (uint16_t)0, nodes[parent].child, (uint16_t)0, a << 24, term << 24};
    nodes[parent].child = (uint16_t)at;
}

// Step 3 of a leaf that the move into it decided: all P outcomes at once, as wins | losses << 16
__device__ __forceinline__ uint32_t tree_decided(uint32_t term, uint32_t P)
{
    return term == kTreeWon ? P : (term == kTreeLost ? P << 16 : 0u);
}

// One ply of a leaf's playout: ply index t = 0 plays nothing (word 0 of a playout id belongs to the expansion), t >= 1 is
// playout_ply.  The outcome counts for the side that moved INTO the leaf (1 - side0); PlayoutEnd.plies = masked-random plies played.
__device__ __forceinline__ PlayoutEnd tree_playout_ply(Planes &p, int &side, int side0, uint32_t t, uint32_t word, uint32_t max_plies)
{
    const int w = t ? playout_ply(p, side, t, 0, word) : 0;
    PlayoutEnd e = playout_end(w, t, 1 - side0, max_plies);
    e.plies -= 1u;  // (playout_end counts a root move; here there is none)
    return e;
}

// One whole playout of a leaf (the host flavour; k_tree deals the P playouts to its lanes)
__device__ __forceinline__ PlayoutEnd tree_playout(const Planes &leaf, int side0, uint64_t seed, uint64_t pid, uint32_t call,
                                                   uint32_t max_plies)
{
    Planes p = leaf;
    int side = side0;
    Draw4 d{};
    for (uint32_t t = 0;; ++t) {
        if ((t & 3u) == 0) d = draw_block(seed, pid, playout_ply_index(call, t), kStreamTree);
        const PlayoutEnd e = tree_playout_ply(p, side, side0, t, draw_word(d, t), max_plies);
        if (e.done) return e;
    }
}

// Step 4: from the leaf to the root, the two counts swapping sides at every level; the root only counts visits
__device__ __forceinline__ void tree_backup(TreeNode *nodes, uint32_t leaf, uint32_t wins, uint32_t losses)
{
    for (uint32_t v = leaf; v; v = nodes[v].parent) {
        nodes[v].n += 1;
        nodes[v].w += wins;
        nodes[v].l += losses;
        const uint32_t x = wins;
        wins = losses;
        losses = x;
    }
    nodes[0].n += 1;
}

// ---- gbl_collect_search: whole games with the tree search on either side (contract: include/gobblet_hip.h) --
constexpr int kPolicyTree = 4;                 // GBL_POLICY_TREE
constexpr int kPolicyEvalTree = 5;             // GBL_POLICY_EVAL_TREE (gbl_collect_search_eval)
constexpr int kHowSearch = 3, kHowSearchSampled = 4;  // GBL_HOW_SEARCH / GBL_HOW_SEARCH_SAMPLED (0 = GBL_HOW_RANDOM)
constexpr int kHowProven = 5;                  // GBL_HOW_PROVEN (gbl_collect_search_solve)
constexpr int kPolicyTablebase = 6;            // GBL_POLICY_TABLEBASE (gbl_collect_search_tb)
constexpr int kHowTable = 6, kHowTableSampled = 7;  // GBL_HOW_TABLE / GBL_HOW_TABLE_SAMPLED
constexpr int kTbTargetResult = 0, kTbTargetShortest = 1;  // GBL_TB_TARGET_RESULT / _SHORTEST (gbl_tb_targets, gbl_collect_search_tb)
constexpr int kTbTargetMaxCount = 600;
constexpr int kZOpen = -128;                   // GBL_Z_OPEN
constexpr uint32_t kStreamVisit = 4u;          // generator stream of the visit-proportional draw of a game's first plies

// The visit-proportional draw on generator word r: k = (r * S) >> 32 with S the sum of the visits, then the lowest action whose
// running sum of visits exceeds k; -1 when nothing was visited.  (One action after the other: the host flavour; the kernel takes a
// prefix sum over the lanes, k_collect_search.)
__device__ __forceinline__ int visits_pick(const int32_t (&visits)[kActions], uint32_t r)
{
    uint32_t S = 0, run = 0;
    for (int a = 0; a < kActions; ++a) S += (uint32_t)visits[a];
    const uint32_t k = __umulhi(r, S);
    for (int a = 0; a < kActions; ++a) {
        run += (uint32_t)visits[a];
        if (run > k) return a;
    }
    return -1;
}

// ---- gbl_evaluate / gbl_tree_search_eval: the integer network and the search it guides (contract: include/gobblet_hip.h) --
// Every step is a function of one hidden-unit quad / one output / one action, so that the kernels give a lane each and the host
// flavour runs them one after the other: the same arithmetic, bit for bit.  Every operand stays inside int32.
constexpr int kEvalOutputs = 56, kEvalValue = 54;  // outputs 0..53: the action logits, 54: the value, 55: padding
constexpr int kEvalMaxHidden = 256, kEvalMaxShift = 24;
constexpr int kTreeEvalMaxIterations = 512;
constexpr uint32_t kTreeEvalP = 128u;  // a network leaf counts as 128 games: q is in 1/128 of a win

struct EvalNet {  // gbl_evaluator, as the kernels take it (by value)
    const int8_t *w1;
    const int32_t *b1;
    const int8_t *w2;
    const int32_t *b2;
    int32_t hidden, shift1, shift_p, shift_v;
};

__device__ __forceinline__ uint32_t eval_load4(const int8_t *w)  // four weights as one dword (w is 4-byte aligned)
{
#ifndef GBL_HOST_EMU
    return *reinterpret_cast<const uint32_t *>(w);
#else
    uint32_t x;
    __builtin_memcpy(&x, w, 4);
    return x;
#endif
}

// acc + the dot product of four signed bytes with four signed bytes: v_dot4_i32_i8
__device__ __forceinline__ int32_t eval_dot4(uint32_t a, uint32_t b, int32_t acc)
{
#ifndef GBL_HOST_EMU
    return __builtin_amdgcn_sdot4((int)a, (int)b, acc, false);
#else
    for (int u = 0; u < 4; ++u) acc += (int32_t)(int8_t)(a >> (8 * u)) * (int32_t)(int8_t)(b >> (8 * u));
    return acc;
#endif
}

__device__ __forceinline__ int32_t eval_clamp(int32_t x, int32_t lo, int32_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Layer 1, hidden units j0 .. j0 + 3 (j0 a multiple of 4) of position p as `side` observes it: the sum of the weight rows of the
// set observation bytes (obs_scatter_row's rule: byte 13 pos + ch; at most 12 pieces, and the 9 bytes of channel 12 when player_2
// observes), never a matrix product.  Returns h as four bytes, unit j0 lowest.
__device__ __forceinline__ uint32_t eval_hidden4(const EvalNet &net, const Planes &p, int side, uint32_t j0)
{
    const uint32_t pos = p.nz & ~p.neg, ngv = p.nz & p.neg;
    const uint32_t own = side ? ngv : pos, opp = side ? pos : ngv;
    const uint32_t X[4] = {own & p.odd, own & ~p.odd, opp & p.odd, opp & ~p.odd};
    const int8_t *col = net.w1 + j0;
    int32_t acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = net.b1[j0 + u];
    // Straight-line code, every load issued before the first sum needs one: a piece that is not on the board reads the row of
    // square 8 of its own channel, channel 12 is read whoever observes, and the dword is dropped afterwards.
    uint32_t rows[21];
#pragma unroll
    for (int ch = 0; ch < 12; ++ch) {
        const int k = (ch % 6) / 2;
        const uint32_t grp = (X[(ch < 6 ? 0 : 2) + (ch & 1)] >> (9 * k)) & 0x1FFu;
        const uint32_t row = eval_load4(col + (13 * __builtin_ctz(grp | 0x100u) + ch) * net.hidden);
        rows[ch] = grp ? row : 0u;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        const uint32_t row = eval_load4(col + (13 * q + 12) * net.hidden);
        rows[12 + q] = side ? row : 0u;
    }
#pragma unroll
    for (int r = 0; r < 21; ++r) {
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += (int32_t)(int8_t)(rows[r] >> (8 * u));
    }
    uint32_t h = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) h |= (uint32_t)eval_clamp(acc[u] >> net.shift1, 0, 127) << (8 * u);
    return h;
}

// all H hidden units, into h4[H / 4] (the host flavour; the kernels give every quad a lane)
__device__ __forceinline__ void eval_hidden(const EvalNet &net, const Planes &p, int side, uint32_t *h4)
{
    for (uint32_t j0 = 0; j0 < (uint32_t)net.hidden; j0 += 4) h4[j0 >> 2] = eval_hidden4(net, p, side, j0);
}

// Layer 2, output k < 56: b2_k + sum_j h_j w2(j, k), four hidden units per step (h <= 127, so both operands are signed bytes)
__device__ __forceinline__ int32_t eval_output(const EvalNet &net, const uint32_t *h4, uint32_t k)
{
    int32_t o = net.b2[k];
    const int8_t *w = net.w2 + 4u * k;
    const int quads = net.hidden >> 2;
#pragma unroll 8
    for (int j = 0; j < quads; ++j) o = eval_dot4(eval_load4(w + j * 4 * kEvalOutputs), h4[j], o);
    return o;
}

__device__ __forceinline__ void eval_outputs(const EvalNet &net, const uint32_t *h4, int32_t (&o)[kEvalOutputs])
{
    for (uint32_t k = 0; k < (uint32_t)kEvalOutputs; ++k) o[k] = eval_output(net, h4, k);
}

__device__ __forceinline__ int32_t eval_value(const EvalNet &net, int32_t o54) { return eval_clamp(o54 >> net.shift_v, -128, 128); }

// 2^(-d / 16) in 1/65536, d = the distance of a logit below the largest one, capped at 255 (16 octaves)
__device__ __forceinline__ uint32_t eval_exp2(int32_t lmax, int32_t l)
{
    constexpr uint32_t T[16] = {65536u, 62757u, 60097u, 57549u, 55109u, 52773u, 50535u, 48393u,
                                46341u, 44376u, 42495u, 40693u, 38968u, 37316u, 35734u, 34219u};
    const int32_t d = lmax - l < 255 ? lmax - l : 255;
    return T[d & 15] >> (d >> 4);
}
__device__ __forceinline__ uint32_t eval_prior(uint32_t e, uint32_t sum) { return 1u + (e * 254u) / sum; }  // (sum >= e, sum > 0)

// the prior row of a candidate set (the host flavour; the kernels take the maximum and the sum over the wavefront)
__device__ __forceinline__ void eval_priors(const EvalNet &net, const int32_t (&o)[kEvalOutputs], uint64_t cand, uint8_t *pri)
{
    int32_t lmax = INT32_MIN;
    for (int a = 0; a < kActions; ++a)
        if (((cand >> a) & 1ull) && (o[a] >> net.shift_p) > lmax) lmax = o[a] >> net.shift_p;
    uint32_t sum = 0;
    for (int a = 0; a < kActions; ++a)
        if ((cand >> a) & 1ull) sum += eval_exp2(lmax, o[a] >> net.shift_p);
    for (int a = 0; a < kActions; ++a) pri[a] = (uint8_t)(((cand >> a) & 1ull) ? eval_prior(eval_exp2(lmax, o[a] >> net.shift_p), sum) : 0u);
}

// ---- root noise (include/gobblet_hip.h, "Root noise"): one statement for the kernels and the host flavour ---------------------
// The noise row is the prior rule itself (eval_exp2 / eval_prior) over logits l_a = -(r_a >> 24), r_a a generator word of its own
// stream.  The kernels give every action a lane and take the maximum and the sum over the wavefront; the host flavour runs
// noise_priors.
constexpr uint32_t kStreamNoise = 6u;  // generator stream of the root noise
constexpr int kNoiseMaxWeight = 256;

// l_a: minus the top byte of the word of (seed, g, ply index 64 q + a) -- one Philox block serves four actions
__device__ __forceinline__ int32_t noise_logit(uint64_t seed, uint64_t g, uint32_t q, uint32_t a)
{
    return -(int32_t)(draw32(seed, g, 64u * q + a, kStreamNoise) >> 24);
}

__device__ __forceinline__ uint32_t noise_mix(uint32_t pi, uint32_t nu, uint32_t w) { return (pi * (256u - w) + nu * w + 128u) >> 8; }

// pri: the root's prior row pi over cand (cand != 0, 0 < w <= 256); mixed: pi' (may be pri itself)
__device__ __forceinline__ void noise_priors(uint64_t seed, uint64_t g, uint32_t q, uint32_t w, uint64_t cand, const uint8_t *pri, uint8_t *mixed)
{
    int32_t l[kActions], lmax = INT32_MIN;
    uint32_t sum = 0;
    for (int a = 0; a < kActions; ++a) {
        if (!((cand >> a) & 1ull)) continue;
        l[a] = noise_logit(seed, g, q, (uint32_t)a);
        if (l[a] > lmax) lmax = l[a];
    }
    for (int a = 0; a < kActions; ++a)
        if ((cand >> a) & 1ull) sum += eval_exp2(lmax, l[a]);
    for (int a = 0; a < kActions; ++a)
        mixed[a] = (uint8_t)(((cand >> a) & 1ull) ? noise_mix(pri[a], eval_prior(eval_exp2(lmax, l[a]), sum), w) : 0u);
}

inline const char *noise_error(int noise) { return noise < 0 || noise > kNoiseMaxWeight ? "the noise weight must be in [0, 256]" : nullptr; }

// ---- playout cap (include/gobblet_hip.h, gbl_collect_search_cap): one statement for the kernel and the host flavour -----------------
// Ply q of board g is FULL iff the top byte of its word on the cap's own stream lies below the mover's share (in 1/256); a full ply
// searches with the side's budget and noise weight, a fast one with the fast budget and weight 0 (no noise: nothing of it is drawn).
// A share of 256 draws nothing.  Every argument is the same in all lanes of a board's wavefront, and so is the result.
constexpr uint32_t kStreamCap = 9u;  // generator stream of the playout cap's draw
constexpr int kCapFullShare = 256;
constexpr int kHowFast = 8, kHowFastSampled = 9;  // GBL_HOW_FAST / GBL_HOW_FAST_SAMPLED

struct CapPly {
    bool fast;
    uint32_t its, noise;
};

__device__ __forceinline__ bool cap_full(uint64_t seed, uint64_t g, uint32_t q, uint32_t share)
{
    return share >= (uint32_t)kCapFullShare || (draw32(seed, g, q, kStreamCap) >> 24) < share;
}

__device__ __forceinline__ CapPly cap_ply(uint64_t seed, uint64_t g, uint32_t q, uint32_t share, uint32_t iterations, uint32_t fast_iterations,
                                          uint32_t noise)
{
    const bool full = cap_full(seed, g, q, share);
    return CapPly{!full, full ? iterations : fast_iterations, full ? noise : 0u};
}

// a side's share and fast budget, where they are read (an EVAL_TREE side; the budget where the share is below 256)
inline const char *cap_share_error(int share) { return share < 0 || share > kCapFullShare ? "full_share0 / full_share1 must be in [0, 256]" : nullptr; }
inline const char *cap_fast_error(int fast_iterations, int iterations)
{
    return fast_iterations < 1 || fast_iterations > iterations ? "fast_iterations0 / fast_iterations1 must be in [1, iterations]" : nullptr;
}

// The selection key of candidate a with prior pi under a node of nv visits: the mean of its child (tree_key's first term; 32768
// without a child, n = 0) plus ((explore pi isqrt(nv << 8)) >> 5) / (1 + n).  nv <= 512: the root of the isqrt stays below 2^24,
// the product below 1024 * 255 * 363 < 2^27.
__device__ __forceinline__ uint32_t tree_eval_mean(uint32_t W, uint32_t L, uint32_t n)  // (n >= 1) 0 .. 65536, for the side that moved into the child
{
    const uint32_t d = n * kTreeEvalP, x = W + d - L;
    const uint32_t hi = (x << 7) / d, rem = (x << 7) - hi * d;
    return (hi << 8) + (rem << 8) / d;
}

__device__ __forceinline__ uint32_t tree_eval_key(bool child, uint32_t W, uint32_t L, uint32_t n, uint32_t nv, uint32_t pi, uint32_t explore)
{
    const uint32_t mean = child ? tree_eval_mean(W, L, n) : 32768u;
    return mean + ((explore * pi * tree_isqrt(nv << 8)) >> 5) / (1u + (child ? n : 0u));
}

// the outcome of a network leaf for the side that moved INTO it, as wins | losses << 16 (q: for the side to move at the leaf)
__device__ __forceinline__ uint32_t tree_eval_outcome(int32_t q) { return q < 0 ? (uint32_t)-q : (uint32_t)q << 16; }

// Where an iteration's selection stopped: at `node` with position p, `side` to move.  expand: action `a` of the node has no child
// and is the expansion; otherwise the node is terminal and is evaluated itself.
struct TreeEvalLeaf {
    uint32_t node;
    Planes p;
    int side;
    bool expand;
    uint32_t a;
};

// Selection, one node and one candidate after the other (the host flavour; k_tree_eval gives every action a lane).  pri: the prior
// rows, kEvalOutputs bytes per node.  rootcand != 0.  root_action >= 0: the root takes that action whatever its keys say (the Gumbel
// root rule picks it, gumbel_root_select); below the root nothing changes.
__device__ __forceinline__ TreeEvalLeaf tree_eval_select(const TreeNode *nodes, const uint8_t *pri, const Planes &root, int mover,
                                                         uint64_t rootcand, uint32_t explore, int root_action = -1)
{
    TreeEvalLeaf s{0u, root, mover, false, 0u};
    uint64_t cand = rootcand;
    for (;;) {
        const TreeNode v = nodes[s.node];
        if (tree_term(v)) return s;
        uint32_t of[kActions] = {};
        for (uint32_t c = v.child; c; c = nodes[c].sibling) of[tree_action(nodes[c])] = c;
        uint32_t best = 0;
        for (uint32_t a = 0; a < (uint32_t)kActions; ++a) {
            if (!((cand >> a) & 1ull)) continue;
            const TreeNode k = nodes[of[a]];  // (of[a] == 0: the root, not looked at)
            const uint32_t key = tree_order_key(tree_eval_key(of[a] != 0, tree_wins(k), tree_losses(k), k.n, v.n,
                                                              pri[s.node * kEvalOutputs + a], explore), a);
            if (key > best) best = key;
        }
        s.a = s.node == 0u && root_action >= 0 ? (uint32_t)root_action : 63u - (best & 63u);
        if (!of[s.a]) {
            s.expand = true;
            return s;
        }
        move_planes(s.p, s.side, s.a);
        s.side ^= 1;
        s.node = of[s.a];
        cand = legal54(s.p, s.side);
    }
}

// ---- Gumbel root search (include/gobblet_hip.h, "Gumbel root search"): one statement for the kernels and the host flavour ---------
// The scalar pieces -- the draw, the root logit, the completed value, sigma, the schedule and the three order keys -- are functions of
// one action, so that the kernels give every action a lane (the considered set A is a ballot mask, "the k largest" a count over the
// set bits) and the host flavour runs them one after the other (GumbelRoot below).
constexpr uint32_t kStreamGumbel = 10u;  // generator stream of the Gumbel row
constexpr int kGumbelMaxConsidered = 54, kGumbelMaxOffset = 255, kGumbelMaxScale = 64;
constexpr int kHowGumbel = 10;  // GBL_HOW_GUMBEL

struct GumbelArgs {  // considered == 0: the side searches by gbl_tree_search_eval's rule (the self-play entry points with the rule alone admit it)
    uint32_t considered, noise, visit_offset, scale;
};

// g_a: the table at the top byte of the word of (seed, g, ply index 64 q + a) -- one Philox block serves four actions
__device__ __forceinline__ int32_t gumbel_draw(uint64_t seed, uint64_t g, uint32_t q, uint32_t a)
{
    return kGumbelTable[draw32(seed, g, 64u * q + a, kStreamGumbel) >> 24];
}

// the root logit: minus the distance below the largest one, the prior rule's own cap
__device__ __forceinline__ int32_t gumbel_logit(int32_t lmax, int32_t l) { return -(lmax - l < 255 ? lmax - l : 255); }

// the completed value of an action: its child's mean, else the root's q on the same 0 .. 65536 scale
__device__ __forceinline__ uint32_t gumbel_mean(bool child, uint32_t W, uint32_t L, uint32_t n, int32_t q_root)
{
    return child ? tree_eval_mean(W, L, n) : (uint32_t)(32768 + 256 * q_root);
}

// sigma: (767 * 64 * 65536 < 2^32)
__device__ __forceinline__ int32_t gumbel_sigma(const GumbelArgs &G, uint32_t maxN, uint32_t mean)
{
    return (int32_t)(((G.visit_offset + maxN) * G.scale * mean) >> 16);
}

__device__ __forceinline__ uint32_t gumbel_phases(uint32_t m)  // max(1, ceil(log2 m)), m >= 1
{
    uint32_t p = 0;
    while ((1u << p) < m) ++p;
    return p ? p : 1u;
}
__device__ __forceinline__ uint32_t gumbel_step(uint32_t iterations, uint32_t P, uint32_t k)
{
    const uint32_t s = iterations / (P * k);
    return s ? s : 1u;
}
__device__ __forceinline__ uint32_t gumbel_kept(uint32_t k) { return k <= 4u ? 2u : (k + 1u) >> 1; }  // max(2, ceil(k / 2)), k > 2

// The order keys, each a max: 0 stands for an action outside the set.  s = g + l (>= -42 - 255) or g + l + sigma (< 2^16 - 512).
//   rank: the larger s, then the lower action -- the considered set and the halving
//   pick: the fewest visits (n <= 512), then the larger g + l, then the lower action -- the root's selection
//   final: the most visits, then the larger g + l + sigma, then the lower action -- the decision
__device__ __forceinline__ uint32_t gumbel_rank_key(int32_t s, uint32_t a) { return ((uint32_t)(s + 512) << 6) | (63u - a); }
__device__ __forceinline__ uint32_t gumbel_pick_key(uint32_t n, int32_t gl, uint32_t a) { return ((512u - n) << 16) | gumbel_rank_key(gl, a); }
__device__ __forceinline__ uint32_t gumbel_final_key(uint32_t n, int32_t s, uint32_t a) { return (n << 22) | gumbel_rank_key(s, a); }
__device__ __forceinline__ int gumbel_action_of(uint32_t key) { return key ? 63 - (int)(key & 63u) : -1; }

// the k actions of A with the largest keys (the keys differ: each holds its action)
__device__ __forceinline__ uint64_t gumbel_keep(const uint32_t (&key)[kActions], uint64_t A, uint32_t k)
{
    uint64_t kept = 0;
    for (uint64_t i = A; i; i &= i - 1) {
        const int a = __builtin_ctzll(i);
        uint32_t above = 0;
        for (uint64_t j = A; j; j &= j - 1) above += key[__builtin_ctzll(j)] > key[a];
        if (above < k) kept |= 1ull << a;
    }
    return kept;
}

// One root's rule, one action after the other (the host flavour; the kernels keep gum / gl in a lane each and A, T wave-uniform).
struct GumbelRoot {
    GumbelArgs G;
    uint32_t iterations, P, T;
    int32_t q_root;
    uint64_t cand, A;
    int32_t gum[kActions], gl[kActions];
};

// the root's children as the rule reads them: n_a (0 without a child) and mean_a; returns maxN
__device__ __forceinline__ uint32_t gumbel_children(const GumbelRoot &R, const TreeNode *nodes, uint32_t (&n)[kActions], uint32_t (&mean)[kActions])
{
    uint32_t maxN = 0;
    for (int a = 0; a < kActions; ++a) {
        n[a] = 0;
        mean[a] = gumbel_mean(false, 0u, 0u, 1u, R.q_root);
    }
    for (uint32_t c = nodes[0].child; c; c = nodes[c].sibling) {
        const TreeNode &k = nodes[c];
        const uint32_t a = tree_action(k);
        n[a] = k.n;
        mean[a] = gumbel_mean(true, tree_wins(k), tree_losses(k), k.n, R.q_root);
        maxN = k.n > maxN ? k.n : maxN;
    }
    return maxN;
}

// o: the root evaluation's outputs; cand != 0
__device__ __forceinline__ void gumbel_root_init(GumbelRoot &R, const GumbelArgs &G, uint32_t iterations, uint64_t seed, uint64_t g, uint32_t q,
                                                 uint64_t cand, const int32_t (&o)[kEvalOutputs], int32_t shift_p, int32_t q_root)
{
    R.G = G;
    R.iterations = iterations;
    R.q_root = q_root;
    R.cand = cand;
    int32_t lmax = INT32_MIN;
    for (int a = 0; a < kActions; ++a)
        if (((cand >> a) & 1ull) && (o[a] >> shift_p) > lmax) lmax = o[a] >> shift_p;
    uint32_t key[kActions];
    for (int a = 0; a < kActions; ++a) {
        const bool in = (cand >> a) & 1ull;
        R.gum[a] = in && G.noise ? gumbel_draw(seed, g, q, (uint32_t)a) : 0;
        R.gl[a] = in ? R.gum[a] + gumbel_logit(lmax, o[a] >> shift_p) : 0;
        key[a] = in ? gumbel_rank_key(R.gl[a], (uint32_t)a) : 0u;
    }
    const uint32_t c = (uint32_t)__builtin_popcountll(cand), m = G.considered < c ? G.considered : c;
    R.A = gumbel_keep(key, cand, m);
    R.P = gumbel_phases(m);
    R.T = gumbel_step(iterations, R.P, m);
}

// before an iteration's selection: halve where the schedule says so, then the root's action
__device__ __forceinline__ int gumbel_root_select(GumbelRoot &R, const TreeNode *nodes)
{
    uint32_t n[kActions], mean[kActions], key[kActions] = {};
    const uint32_t maxN = gumbel_children(R, nodes, n, mean);
    const uint32_t size = (uint32_t)__builtin_popcountll(R.A);
    bool due = size > 2u;
    for (uint64_t i = R.A; i; i &= i - 1) due = due && n[__builtin_ctzll(i)] >= R.T;
    if (due) {
        for (uint64_t i = R.A; i; i &= i - 1) {
            const int a = __builtin_ctzll(i);
            key[a] = gumbel_rank_key(R.gl[a] + gumbel_sigma(R.G, maxN, mean[a]), (uint32_t)a);
        }
        R.A = gumbel_keep(key, R.A, gumbel_kept(size));
        R.T += gumbel_step(R.iterations, R.P, (uint32_t)__builtin_popcountll(R.A));
    }
    uint32_t best = 0;
    for (uint64_t i = R.A; i; i &= i - 1) {
        const int a = __builtin_ctzll(i);
        const uint32_t k = gumbel_pick_key(n[a], R.gl[a], (uint32_t)a);
        best = k > best ? k : best;
    }
    return gumbel_action_of(best);
}

// after the last iteration: the decision, and the target row (54 bytes; may be NULL)
__device__ __forceinline__ int gumbel_root_finish(const GumbelRoot &R, const TreeNode *nodes, uint8_t *target)
{
    uint32_t n[kActions], mean[kActions];
    const uint32_t maxN = gumbel_children(R, nodes, n, mean);
    uint32_t best = 0, sum = 0;
    int32_t t[kActions], tmax = INT32_MIN;
    for (int a = 0; a < kActions; ++a) {
        if (!((R.cand >> a) & 1ull)) continue;
        const int32_t sigma = gumbel_sigma(R.G, maxN, mean[a]);
        t[a] = R.gl[a] - R.gum[a] + sigma;
        tmax = t[a] > tmax ? t[a] : tmax;
        if ((R.A >> a) & 1ull) {
            const uint32_t k = gumbel_final_key(n[a], R.gl[a] + sigma, (uint32_t)a);
            best = k > best ? k : best;
        }
    }
    if (target) {
        for (int a = 0; a < kActions; ++a)
            if ((R.cand >> a) & 1ull) sum += eval_exp2(tmax, t[a]);
        for (int a = 0; a < kActions; ++a) target[a] = (uint8_t)(((R.cand >> a) & 1ull) ? eval_prior(eval_exp2(tmax, t[a]), sum) : 0u);
    }
    return gumbel_action_of(best);
}

inline const char *gumbel_error(int considered, int gumbel_noise, int visit_offset, int scale, int least = 1)
{
    if (considered < least || considered > kGumbelMaxConsidered) return least ? "considered must be in [1, 54]" : "considered0 / considered1 must be in [0, 54]";
    if (gumbel_noise != 0 && gumbel_noise != 1) return "gumbel_noise must be 0 or 1";
    if (visit_offset < 0 || visit_offset > kGumbelMaxOffset) return "visit_offset must be in [0, 255]";
    if (scale < 0 || scale > kGumbelMaxScale) return "scale must be in [0, 64]";
    return nullptr;
}

// ---- gbl_solve: the exact depth-bounded solver (contract: include/gobblet_hip.h) ----------------------------------------------
// A result c is +k (the mover wins at ply k), -k (the mover has lost by ply k) or 0 (unproven); rank orders them: the shortest
// win, then the unproven, then the longest loss.  A node's best result travels as an ORDER KEY, rank + 128 (1 .. 191; 0 = no
// move yet, which reads back as V = 0), so that "the result of largest rank" is an unsigned max -- in a register, or an LDS
// atomic where the lanes of a wavefront share a node.
constexpr int kSolveMaxDepth = 6;  // GBL_SOLVE_MAX_DEPTH
constexpr int kSolveNone = -128;   // GBL_SOLVE_NONE

__device__ __forceinline__ int solve_rank(int c) { return c > 0 ? 64 - c : (c < 0 ? -64 - c : 0); }
__device__ __forceinline__ uint32_t solve_key(int c) { return (uint32_t)(solve_rank(c) + 128); }
__device__ __forceinline__ int solve_of_key(uint32_t key)  // V of the node whose best key this is (rank is its own inverse)
{
    return key ? solve_rank((int)key - 128) : 0;
}
// c(a) where nobody has won after a: from u = V of the position after a, for the other side
__device__ __forceinline__ int solve_parent(int u) { return u == 0 ? 0 : (u > 0 ? -(u + 1) : 1 - u); }
// c(a) where check_for_winner() = w after side s played a: s won, s lost at once (it uncovered a line), or 0 = nobody yet
__device__ __forceinline__ int solve_now(int w, int s) { return w == 0 ? 0 : (w == (s ? -1 : 1) ? 1 : -1); }

// The window cut every level shares.  A node's best order key so far is `best`; what is the deepest its NEXT quiet move need be
// searched (plies below that move, at most `left`)?  A quiet move gives +2 at best (every answer of the other side loses at
// once), so a best of +2 settles the node: 0.  A best of +k, k >= 3, is outranked by a +j with j < k alone, and a +j shows with
// j - 1 plies below the move: k - 2 of them are enough.  A shallower search can only turn a result into 0 (a proven result is
// the same at every depth that proves it), and 0 ranks below every win -- so the node's best key, the only thing kept, is that of
// the full-width definition.  A best that is no win cuts nothing.
__device__ __forceinline__ int solve_plies_needed(uint32_t best, int left)
{
    const int k = 192 - (int)best;  // best = solve_key(+k)
    return k >= 2 && k - 2 < left ? k - 2 : left;
}

// V(p, s, r), 1 <= r <= MAXR: the recursion unrolled MAXR levels deep by the template parameter (every level inlined once: no call,
// no stack), r the run-time bound that stops it earlier.  Two passes over a node's moves, which change no value:
//   1. every move played and check_for_winner() read: a win at once ends the node (nothing ranks above +1); the moves after which
//      nobody has won are the `quiet` ones;
//   2. the quiet moves searched r - 1 plies deep, or as deep as solve_plies_needed() says once one of them wins.
template <int MAXR>
__device__ __forceinline__ int solve_value(const Planes &p, int s, int r)
{
    uint64_t quiet = 0;
    uint32_t best = 0;
    for (uint64_t l = legal54(p, s); l; l &= l - 1) {
        const uint32_t a = (uint32_t)__builtin_ctzll(l);
        Planes q = p;
        move_planes(q, s, a);
        const int c = solve_now(winner_of(q), s);
        if (c > 0) return 1;
        if (c < 0) best = solve_key(-1);
        else quiet |= 1ull << a;
    }
    if (!quiet) return solve_of_key(best);
    if (r <= 1) return 0;  // (a quiet move is unproven, which outranks every loss)
    if constexpr (MAXR > 1) {
        for (uint64_t l = quiet; l; l &= l - 1) {
            Planes q = p;
            move_planes(q, s, (uint32_t)__builtin_ctzll(l));
            const int left = solve_plies_needed(best, r - 1);
            if (left == 0) break;
            const uint32_t k = solve_key(solve_parent(solve_value<MAXR - 1>(q, s ^ 1, left)));
            best = k > best ? k : best;
        }
        return solve_of_key(best);
    } else {
        return 0;  // (r <= MAXR: not reached)
    }
}

// The root's first two plies, which the kernel's lanes share and the host flavour walks in the same order.  Root action a of
// `mover`, `depth` plies in all: c is final unless `deep` is non-empty.  Then nobody has won after a, no reply wins at once, and
// `deep` holds the quiet replies, each worth solve_reply(); key is the best of the replies that lose at once (0: none).  When
// every deep reply's key has been folded into key by max, c(a) = solve_parent(solve_of_key(key)).
struct SolveRoot {
    int c;
    uint32_t key;
    uint64_t deep;
};

__device__ __forceinline__ SolveRoot solve_root_action(const Planes &root, int mover, uint32_t a, int depth)
{
    Planes q = root;
    move_planes(q, mover, a);
    SolveRoot R{solve_now(winner_of(q), mover), 0u, 0ull};
    if (R.c != 0 || depth == 1) return R;
    const int other = mover ^ 1;
    for (uint64_t l = legal54(q, other); l; l &= l - 1) {
        const uint32_t b = (uint32_t)__builtin_ctzll(l);
        Planes t = q;
        move_planes(t, other, b);
        const int cb = solve_now(winner_of(t), other);
        if (cb > 0) {  // the reply wins at once: a loses in two
            R.c = -2;
            R.deep = 0;
            return R;
        }
        if (cb < 0) R.key = solve_key(-1);
        else R.deep |= 1ull << b;
    }
    if (depth == 2 && R.deep) {  // the quiet replies are unproven
        R.key = solve_key(0);
        R.deep = 0;
    }
    if (!R.deep) R.c = solve_parent(solve_of_key(R.key));
    return R;
}

// the order key of the quiet reply b to root action a (depth >= 3): the lane's serial part, depth - 2 plies from the root's mover.
// `best` is the action's key so far (the max over its replies done): solve_plies_needed() cuts by it as inside solve_value, and a
// reply that needs no ply returns 0, which changes no max.  An OLDER (smaller) best than the action has by now only costs work:
// the cut is exact for every best the action has held.
__device__ __forceinline__ uint32_t solve_reply(const Planes &root, int mover, uint32_t a, uint32_t b, int depth, uint32_t best)
{
    const int left = solve_plies_needed(best, depth - 2);
    if (left == 0) return 0u;
    Planes q = root;
    move_planes(q, mover, a);
    move_planes(q, mover ^ 1, b);
    return solve_key(solve_parent(solve_value<kSolveMaxDepth - 2>(q, mover, left)));
}

// the decision over the root's 54 results: the key of candidate a with result c (0 stands for a non-candidate), the max decides
__device__ __forceinline__ uint32_t solve_action_key(int c, uint32_t a) { return (solve_key(c) << 6) | (63u - a); }
__device__ __forceinline__ int solve_action_of(uint32_t best) { return best ? 63 - (int)(best & 63u) : -1; }
__device__ __forceinline__ int solve_value_of(uint32_t best) { return solve_of_key(best >> 6); }

// ---- argument checks of the search entry points and the trajectory strides: host code, for both flavours of the ABI ----------
// Each *_error returns the message of the first rule the arguments break, or nullptr; a flavour passes it to its own fail().
inline const char *tree_budget_error(int iterations, int playouts)
{
    if (iterations < 1 || iterations > kTreeMaxIterations) return "iterations must be in [1, 1024]";
    if (playouts < 1 || playouts > kTreeMaxPlayouts) return "playouts must be in [1, 256]";
    return nullptr;
}

inline const char *playout_limits_error(int max_plies, int explore = 0)  // (gbl_playout_values has no explore)
{
    if (max_plies < 0 || max_plies > 255) return "max_plies must be in [0, 255]";
    if (explore < 0 || explore > kTreeMaxExplore) return "explore must be in [0, 1024]";
    return nullptr;
}

// the checks of a gbl_evaluator's scalar fields (its four pointers are looked at after the n == 0 return)
template <typename Ev>
inline const char *evaluator_error(const Ev *ev)
{
    if (!ev) return "ev must not be NULL";
    if (ev->hidden != 64 && ev->hidden != 128 && ev->hidden != 192 && ev->hidden != 256) return "hidden must be 64, 128, 192 or 256";
    if (ev->shift1 < 0 || ev->shift1 > kEvalMaxShift || ev->shift_p < 0 || ev->shift_p > kEvalMaxShift || ev->shift_v < 0 ||
        ev->shift_v > kEvalMaxShift)
        return "shift1 / shift_p / shift_v must be in [0, 24]";
    return nullptr;
}
template <typename Ev>
inline const char *evaluator_pointers_error(const Ev *ev)
{
    return ev->w1 && ev->b1 && ev->w2 && ev->b2 ? nullptr : "the evaluator's w1 / b1 / w2 / b2 must not be NULL";
}

inline const char *tree_eval_budget_error(int iterations, int explore)
{
    if (iterations < 1 || iterations > kTreeEvalMaxIterations) return "iterations must be in [1, 512]";
    if (explore < 0 || explore > kTreeMaxExplore) return "explore must be in [0, 1024]";
    return nullptr;
}

inline const char *env_range_error(uint64_t env_base, int64_t n)  // (n >= 0)
{
    return env_base > (1ull << 42) || (uint64_t)n > (1ull << 42) - env_base ? "env_base + n must not exceed 2^42" : nullptr;
}

// what the nine self-play entry points ask of the window: after the policies' own checks
inline const char *selfplay_window_error(int sample_plies, bool has_turn, uint32_t ply0, uint32_t plies, uint64_t env_base, int64_t n)
{
    if (sample_plies < 0) return "sample_plies < 0";
    if (sample_plies > 0 && !has_turn) return "sample_plies > 0 needs the per-board turn counter (turn must not be NULL)";
    if ((uint64_t)ply0 + plies > (1ull << 24)) return "ply0 + plies must not exceed 2^24 (the search's call index)";
    return env_range_error(env_base, n);
}

inline const char *illegal_mode_error(int illegal_mode)
{
    return illegal_mode != 0 && illegal_mode != 1 ? "illegal_mode must be GBL_ILLEGAL_NOOP or GBL_ILLEGAL_TERMINATE" : nullptr;
}

// gbl_collect_search, everything that is looked at before a pointer is: the policies, the searching sides' budgets (a RANDOM side's
// are not read), the playout limits, then the window.  (n >= 0)
inline const char *collect_search_error(int illegal_mode, int policy0, int policy1, int iterations0, int iterations1, int playouts0,
                                        int playouts1, int max_plies, int explore, int sample_plies, bool has_turn, uint32_t ply0,
                                        uint32_t plies, uint64_t env_base, int64_t n)
{
    if (const char *why = illegal_mode_error(illegal_mode)) return why;
    if ((policy0 != 0 && policy0 != kPolicyTree) || (policy1 != 0 && policy1 != kPolicyTree))
        return "policy0 / policy1: GBL_POLICY_RANDOM or GBL_POLICY_TREE";
    if (policy0 == kPolicyTree)
        if (const char *why = tree_budget_error(iterations0, playouts0)) return why;
    if (policy1 == kPolicyTree)
        if (const char *why = tree_budget_error(iterations1, playouts1)) return why;
    if (const char *why = playout_limits_error(max_plies, explore)) return why;
    return selfplay_window_error(sample_plies, has_turn, ply0, plies, env_base, n);
}

// gbl_collect_search_eval, the same: the policies, the searching sides' evaluator and budget (a RANDOM side's are not read), then the
// window.  (n >= 0)
template <typename Ev>
inline const char *collect_eval_error(int illegal_mode, int policy0, int policy1, const Ev *ev0, const Ev *ev1, int iterations0,
                                      int iterations1, int explore, int sample_plies, bool has_turn, uint32_t ply0, uint32_t plies,
                                      uint64_t env_base, int64_t n)
{
    if (const char *why = illegal_mode_error(illegal_mode)) return why;
    if ((policy0 != 0 && policy0 != kPolicyEvalTree) || (policy1 != 0 && policy1 != kPolicyEvalTree))
        return "policy0 / policy1: GBL_POLICY_RANDOM or GBL_POLICY_EVAL_TREE";
    const Ev *evs[2] = {ev0, ev1};
    const int its[2] = {iterations0, iterations1}, pol[2] = {policy0, policy1};
    for (int m = 0; m < 2; ++m) {
        if (pol[m] != kPolicyEvalTree) continue;
        if (const char *why = evaluator_error(evs[m])) return why;
        if (const char *why = tree_eval_budget_error(its[m], explore)) return why;
    }
    return selfplay_window_error(sample_plies, has_turn, ply0, plies, env_base, n);
}

// gbl_collect_search_solve: collect_eval_error, then the guarded sides' depths (a RANDOM side's is not read; 0 = no guard).  (n >= 0)
template <typename Ev>
inline const char *collect_solve_error(int illegal_mode, int policy0, int policy1, const Ev *ev0, const Ev *ev1, int iterations0,
                                       int iterations1, int solve_depth0, int solve_depth1, int explore, int sample_plies, bool has_turn,
                                       uint32_t ply0, uint32_t plies, uint64_t env_base, int64_t n)
{
    if (const char *why = collect_eval_error(illegal_mode, policy0, policy1, ev0, ev1, iterations0, iterations1, explore, sample_plies,
                                             has_turn, ply0, plies, env_base, n))
        return why;
    if ((policy0 == kPolicyEvalTree && (solve_depth0 < 0 || solve_depth0 > kSolveMaxDepth)) ||
        (policy1 == kPolicyEvalTree && (solve_depth1 < 0 || solve_depth1 > kSolveMaxDepth)))
        return "solve_depth0 / solve_depth1 must be in [0, 6]";
    return nullptr;
}

// ---- one self-play call: the arguments of gbl_collect_search, _eval, _solve, _noise, _cap, _gumbel and _tb and of gbl_collect_gumbel_solve and gbl_collect_gumbel_tb, and the checks both flavours make of them ----
// The 19 trajectory arrays (any may be NULL).
struct SelfplayTraj {
    int32_t *actions;
    int8_t *winner, *reward, *done, *to_move, *mask, *obs;
    int16_t *visits;
    int32_t *value, *nodes;
    int8_t *how, *mover;
    int32_t *root_value;  // (the evaluator search's two: NULL in gbl_collect_search)
    uint8_t *priors;
    int8_t *outcome, *proven;  // (the guard's two: NULL but in gbl_collect_search_solve / _noise / _cap / _tb)
    int8_t *tb_outcome, *tb_value, *tb_played;  // (the table's verdict of every ply: NULL but in gbl_collect_search_tb / gbl_collect_gumbel_tb)
};

enum SelfplayRun { kRunSearch, kRunEval, kRunSolve, kRunTb };  // gbl_collect_search; _eval and _gumbel; _solve, _noise, _cap and gbl_collect_gumbel_solve; _tb and gbl_collect_gumbel_tb

// The union of the nine entry points' arguments; an entry point (gobblet_selfplay_entries.inc, one text for both flavours) fills it,
// leaving 0 / NULL what it does not have, and calls its flavour's one runner.  [0] is player_1's, [1] player_2's.  Ev: gbl_evaluator.
template <typename Ev>
struct SelfplayCall {
    SelfplayRun run;
    int8_t *state, *to_move, *done;
    SelfplayTraj traj;
    int64_t n, ply_stride, tile_stride;
    uint64_t seed, env_base;
    uint32_t ply0;
    const uint32_t *ply_dev;
    uint32_t plies;
    int policy[2];
    const Ev *ev[2];
    int iterations[2], playouts[2], solve_depth[2], noise[2];
    int max_plies, explore, sample_plies, illegal_mode;
    int64_t *counters;
    int32_t *turn;
    // gbl_collect_search_tb's and gbl_collect_gumbel_tb's own (0 / NULL elsewhere): the table as gbl_tb_probe takes it, gbl_tb_targets' mode and count
    const int32_t *inventory;
    const void *aux;
    const int8_t *table;
    int tb_mode, tb_count;
    // gbl_collect_search_cap's own (cap = 0 elsewhere: neither array is read)
    int cap;
    int fast[2], share[2];
    // gbl_collect_search_gumbel's, gbl_collect_gumbel_solve's and gbl_collect_gumbel_tb's own (gumbel = 0 elsewhere: none is read)
    int gumbel;
    int considered[2];
    int gumbel_noise, visit_offset, scale;
};

// how many actions side m's Gumbel root rule considers: 0 (the side searches by gbl_tree_search_eval's rule, or does not search) elsewhere
template <typename Ev>
inline int selfplay_considered(const SelfplayCall<Ev> &c, int m)
{
    return c.gumbel && c.policy[m] == kPolicyEvalTree ? c.considered[m] : 0;
}

// the share of full plies that side m's plies are drawn against: 256 (nothing is drawn) without a cap or for a side that does not search
template <typename Ev>
inline int selfplay_share(const SelfplayCall<Ev> &c, int m)
{
    return c.cap && c.policy[m] == kPolicyEvalTree ? c.share[m] : kCapFullShare;
}

// (the tablebase entry points' look at an inventory: "Exact tablebase" below)
inline const char *tb_inventory_error(const int32_t *inventory)
{
    if (!inventory) return "inventory must not be NULL";
    for (int k = 0; k < 3; ++k)
        if (inventory[k] < 0 || inventory[k] > 2) return "inventory entries must be in [0, 2]";
    return nullptr;
}

// whether a gbl_collect_search_tb / gbl_collect_gumbel_tb call reads the table at all: a side plays from it, or a judge array is given
template <typename Ev>
inline bool selfplay_reads_table(const SelfplayCall<Ev> &c)
{
    return c.run == kRunTb && (c.policy[0] == kPolicyTablebase || c.policy[1] == kPolicyTablebase || c.traj.tb_outcome || c.traj.tb_value ||
                               c.traj.tb_played);
}

// gbl_collect_search_tb, everything that is looked at before a pointer to boards is: the illegal mode, the policies (three here), then
// collect_solve_error with a TABLEBASE side read as a RANDOM one (its evaluator, budget and depth are not read), then the table's
// mode and count and, where the call reads the table, the inventory.  gbl_collect_gumbel_tb (c.gumbel; its depths and weights are 0)
// looks at the mode and the count too only where the call reads the table.  (n >= 0)
template <typename Ev>
inline const char *collect_tb_error(const SelfplayCall<Ev> &c)
{
    if (const char *why = illegal_mode_error(c.illegal_mode)) return why;
    int pol[2];
    for (int m = 0; m < 2; ++m) {
        if (c.policy[m] != 0 && c.policy[m] != kPolicyEvalTree && c.policy[m] != kPolicyTablebase)
            return "policy0 / policy1: GBL_POLICY_RANDOM, GBL_POLICY_EVAL_TREE or GBL_POLICY_TABLEBASE";
        pol[m] = c.policy[m] == kPolicyTablebase ? 0 : c.policy[m];
    }
    if (const char *why = collect_solve_error(c.illegal_mode, pol[0], pol[1], c.ev[0], c.ev[1], c.iterations[0], c.iterations[1],
                                              c.solve_depth[0], c.solve_depth[1], c.explore, c.sample_plies, c.turn != nullptr, c.ply0, c.plies,
                                              c.env_base, c.n))
        return why;
    if (c.gumbel && !selfplay_reads_table(c)) return nullptr;
    if (c.tb_mode != kTbTargetResult && c.tb_mode != kTbTargetShortest) return "tb_mode must be GBL_TB_TARGET_RESULT or GBL_TB_TARGET_SHORTEST";
    if (c.tb_count < 1 || c.tb_count > kTbTargetMaxCount) return "tb_count must be in [1, 600]";
    return selfplay_reads_table(c) ? tb_inventory_error(c.inventory) : nullptr;
}

// Everything both flavours look at, in the order they report it: n < 0, the entry point's *_error, the searching sides' noise
// weights, (gbl_collect_search_cap: their shares, then their fast budgets,) (gbl_collect_search_gumbel, gbl_collect_gumbel_solve, gbl_collect_gumbel_tb: their `considered`, then the
// rule's three where a side follows it,) n == 0, the three board arrays, (gbl_collect_search_tb, gbl_collect_gumbel_tb, where the call reads the table: aux, then table,) plies == 0, then
// per searching side `side(m)` -- the flavour's own look at evaluator m
// (its pointers; on the device their alignment too), which returns 0 or what its fail() returned.  Returns a flavour's error
// code (< 0; fail(message) makes a GBL_ERR_ARG of a message), 0 where there is nothing to do (GBL_OK), or 1: the flavour goes on
// with the strides (and its alignments) and runs.  most: the larger tree of the sides that search.
template <typename Ev, typename Fail, typename Side>
inline int selfplay_prologue(const SelfplayCall<Ev> &c, int &most, Fail &&fail, Side &&side)
{
    const bool uct = c.run == kRunSearch;
    const int searching = uct ? kPolicyTree : kPolicyEvalTree;
    if (c.n < 0) return fail("n < 0");
    const char *why = uct ? collect_search_error(c.illegal_mode, c.policy[0], c.policy[1], c.iterations[0], c.iterations[1], c.playouts[0],
                                                 c.playouts[1], c.max_plies, c.explore, c.sample_plies, c.turn != nullptr, c.ply0, c.plies,
                                                 c.env_base, c.n)
                      : c.run == kRunTb ? collect_tb_error(c)
                          : collect_solve_error(c.illegal_mode, c.policy[0], c.policy[1], c.ev[0], c.ev[1], c.iterations[0], c.iterations[1],
                                                c.solve_depth[0], c.solve_depth[1], c.explore, c.sample_plies, c.turn != nullptr, c.ply0,
                                                c.plies, c.env_base, c.n);
    if (why) return fail(why);
    if (!uct && ((c.policy[0] == searching && noise_error(c.noise[0])) || (c.policy[1] == searching && noise_error(c.noise[1]))))
        return fail("noise0 / noise1 must be in [0, 256]");
    if (c.cap) {  // gbl_collect_search_cap: the searching sides' shares, then the fast budgets that are read
        for (int m = 0; m < 2; ++m)
            if (c.policy[m] == searching)
                if (const char *bad = cap_share_error(c.share[m])) return fail(bad);
        for (int m = 0; m < 2; ++m)
            if (c.policy[m] == searching && c.share[m] < kCapFullShare)
                if (const char *bad = cap_fast_error(c.fast[m], c.iterations[m])) return fail(bad);
    }
    if (c.gumbel) {  // gbl_collect_search_gumbel, gbl_collect_gumbel_solve, gbl_collect_gumbel_tb: the searching sides' considered, then the rule's three where a side follows it
        for (int m = 0; m < 2; ++m)
            if (c.policy[m] == searching)
                if (const char *bad = gumbel_error(c.considered[m], 0, 0, 0, 0)) return fail(bad);
        if (selfplay_considered(c, 0) || selfplay_considered(c, 1))
            if (const char *bad = gumbel_error(kGumbelMaxConsidered, c.gumbel_noise, c.visit_offset, c.scale)) return fail(bad);
    }
    if (c.n == 0) return 0;
    if (!c.state) return fail("state must not be NULL");
    if (!c.to_move) return fail("to_move must not be NULL");
    if (!c.done) return fail("done must not be NULL");
    if (selfplay_reads_table(c)) {
        if (!c.aux) return fail("aux must not be NULL");
        if (!c.table) return fail("table must not be NULL");
    }
    if (c.plies == 0) return 0;
    most = 0;
    for (int m = 0; m < 2; ++m) {
        if (c.policy[m] != searching) continue;  // (a RANDOM side's evaluator and budget are not read)
        if (!uct)
            if (const int e = side(m)) return e;
        most = c.iterations[m] > most ? c.iterations[m] : most;
    }
    return 1;
}

// gbl_solve: every check, in the order both flavours report them.  Returns the message (nullptr: none) and, in `code`, which error
// it is (0 = GBL_ERR_ARG, 1 = GBL_ERR_ALIGN).  n == 0 passes whatever the pointers are: the caller returns GBL_OK before using them.
inline const char *solve_error(int depth, int64_t n, const void *state, const void *to_move, const void *action_out, int &code)
{
    code = 0;
    if (n < 0) return "n < 0";
    if (depth < 1 || depth > kSolveMaxDepth) return "depth must be in [1, 6]";
    if (n == 0) return nullptr;
    if (!state) return "state must not be NULL";
    if (!to_move) return "to_move must not be NULL";
    code = 1;
    if (reinterpret_cast<uintptr_t>(action_out) & 3u) return "action_out must be 4-byte aligned";
    return nullptr;
}

// The other single-decision entry points, likewise: what BOTH flavours look at, in the order they report it (every one a
// GBL_ERR_ARG; n == 0 passes whatever the pointers are).  The device flavour's alignment rules follow there, after these.
inline const char *call_env_error(uint32_t call, uint64_t env_base, int64_t n)  // (n >= 0)
{
    return call >= (1u << 24) ? "call must be below 2^24" : env_range_error(env_base, n);
}

inline const char *boards_error(const void *state, const void *to_move)
{
    return !state ? "state must not be NULL" : !to_move ? "to_move must not be NULL" : nullptr;
}

inline const char *playout_values_error(int playouts, int max_plies, uint32_t call, uint64_t env_base, int64_t n, const void *state,
                                        const void *to_move)
{
    if (n < 0) return "n < 0";
    if (playouts < 1 || playouts > 4096) return "playouts must be in [1, 4096]";
    if (const char *why = playout_limits_error(max_plies)) return why;
    if (const char *why = call_env_error(call, env_base, n)) return why;
    return n == 0 ? nullptr : boards_error(state, to_move);
}

inline const char *tree_search_error(int iterations, int playouts, int max_plies, int explore, uint32_t call, uint64_t env_base, int64_t n,
                                     const void *state, const void *to_move)
{
    if (n < 0) return "n < 0";
    if (const char *why = tree_budget_error(iterations, playouts)) return why;
    if (const char *why = playout_limits_error(max_plies, explore)) return why;
    if (const char *why = call_env_error(call, env_base, n)) return why;
    return n == 0 ? nullptr : boards_error(state, to_move);
}

template <typename Ev>
inline const char *evaluate_error(const Ev *ev, int64_t n, const void *state, const void *to_move, const void *priors_out,
                                  const void *value_out)
{
    if (n < 0) return "n < 0";
    if (const char *why = evaluator_error(ev)) return why;
    if (n == 0) return nullptr;
    if (const char *why = boards_error(state, to_move)) return why;
    if (!priors_out) return "priors_out must not be NULL";
    if (!value_out) return "value_out must not be NULL";
    return evaluator_pointers_error(ev);
}

template <typename Ev>
inline const char *tree_search_eval_error(const Ev *ev, int iterations, int explore, int64_t n, const void *state, const void *to_move)
{
    if (n < 0) return "n < 0";
    if (const char *why = evaluator_error(ev)) return why;
    if (const char *why = tree_eval_budget_error(iterations, explore)) return why;
    if (n == 0) return nullptr;
    if (const char *why = boards_error(state, to_move)) return why;
    return evaluator_pointers_error(ev);
}

// gbl_tree_search_eval_noise's own four, in front of tree_search_eval_error
inline const char *tree_search_noise_error(int noise, uint32_t call, uint64_t env_base, int64_t n)
{
    if (n < 0) return "n < 0";
    if (const char *why = noise_error(noise)) return why;
    return call_env_error(call, env_base, n);
}

// gbl_tree_search_gumbel: gbl_tree_search_eval_noise's errors in their order (the noise weight apart), then the rule's four
template <typename Ev>
inline const char *tree_search_gumbel_error(const Ev *ev, int iterations, int explore, int considered, int gumbel_noise, int visit_offset,
                                            int scale, uint32_t call, uint64_t env_base, int64_t n, const void *state, const void *to_move)
{
    if (const char *why = tree_search_noise_error(0, call, env_base, n)) return why;
    if (const char *why = tree_search_eval_error(ev, iterations, explore, n < 0 ? n : 0, state, to_move)) return why;
    if (const char *why = gumbel_error(considered, gumbel_noise, visit_offset, scale)) return why;
    return tree_search_eval_error(ev, iterations, explore, n, state, to_move);
}

// The (ply, tile) cells of 64 boards of a trajectory must start 16-byte aligned and must not overlap.
inline bool strides_ok(int64_t n, uint32_t plies, int64_t ply_stride, int64_t tile_stride)
{
    const int64_t tiles = (n + kTile - 1) / kTile;
    const bool aligned = ply_stride > 0 && tile_stride > 0 && !(ply_stride & 15) && !(tile_stride & 15);
    const bool time_major = tile_stride >= kTile && (plies == 1 || ply_stride >= (tiles - 1) * tile_stride + kTile);
    const bool tile_major = ply_stride >= kTile && (tiles == 1 || tile_stride >= ((int64_t)plies - 1) * ply_stride + kTile);
    return aligned && (time_major || tile_major);
}
constexpr const char *kStridesMessage = "ply_stride / tile_stride: multiples of 16 boards that keep the (ply, tile) cells apart";

// ---- argument checks of the env, collect and greedy entry points (gbl_reset ... gbl_greedy_act_at): host code, for both flavours ------
// One *_error per entry point that checks anything (gbl_step, _step_into, _sample, _rollout, _collect, _collect_from and _greedy_act
// forward: gobblet_env_entries.inc): every rule BOTH flavours have, in the order they report it, every one a GBL_ERR_ARG.  n == 0 (and,
// where there are plies, plies == 0 once the rules in front of it hold) passes whatever comes after it: the caller returns GBL_OK
// before using anything.  The device flavour's alignment rules follow there, after these.  tests/golden/env_arg_errors.json
// (scripts/record_env_arg_errors.py) pins every rule alone, every adjacent pair and the early returns, on both flavours.
#define GBL_N(n) if ((n) <= 0) return (n) < 0 ? "n < 0" : nullptr
#define GBL_PTR(p) if (!(p)) return #p " must not be NULL"  // (the parameter bears the ABI's name)
inline const char *reset_error(int64_t n, const void *state, const void *to_move, const void *done) { GBL_N(n); GBL_PTR(state); GBL_PTR(to_move); GBL_PTR(done); return nullptr; }
inline const char *legal_mask_error(int64_t n, const void *state, const void *to_move, const void *mask) { GBL_N(n); GBL_PTR(state); GBL_PTR(to_move); GBL_PTR(mask); return nullptr; }
inline const char *is_legal_error(int64_t n, const void *state, const void *agent_index, const void *actions, const void *out) { GBL_N(n); GBL_PTR(state); GBL_PTR(agent_index); GBL_PTR(actions); GBL_PTR(out); return nullptr; }
inline const char *play_turn_error(int64_t n, const void *state, const void *agent_index, const void *actions) { GBL_N(n); GBL_PTR(state); GBL_PTR(agent_index); GBL_PTR(actions); return nullptr; }
inline const char *winner_error(int64_t n, const void *state, const void *winner) { GBL_N(n); GBL_PTR(state); GBL_PTR(winner); return nullptr; }
inline const char *flatboard_error(int64_t n, const void *state, const void *flat) { GBL_N(n); GBL_PTR(state); GBL_PTR(flat); return nullptr; }
inline const char *covered_error(int64_t n, const void *state, const void *cov) { GBL_N(n); GBL_PTR(state); GBL_PTR(cov); return nullptr; }
inline const char *validate_error(int64_t n, const void *state, const void *flags) { GBL_N(n); GBL_PTR(state); GBL_PTR(flags); return nullptr; }
inline const char *sample_error(int64_t n, const void *mask, const void *actions) { GBL_N(n); GBL_PTR(mask); GBL_PTR(actions); return nullptr; }
inline const char *decode_obs_error(int64_t n, const void *obs, const void *state, const void *to_move) { GBL_N(n); GBL_PTR(obs); GBL_PTR(state); GBL_PTR(to_move); return nullptr; }

inline const char *observe_error(int64_t n, const void *state, const void *to_move, int agent_sel, const void *obs)
{
    GBL_N(n); GBL_PTR(state); GBL_PTR(obs);
    if (agent_sel < -1 || agent_sel > 1) return "agent_sel must be -1, 0 or 1";
    return agent_sel < 0 && !to_move ? "to_move (agent_sel == -1) must not be NULL" : nullptr;
}

inline const char *board_eval_error(int64_t n, const void *state, const void *agent_index, const void *actions, const void *record_out)
{
    GBL_N(n); GBL_PTR(state); GBL_PTR(record_out);
    return actions && !agent_index ? "agent_index (with actions) must not be NULL" : nullptr;
}

// the boards a ply is played on, and how an illegal action is taken: gbl_step_ex (which needs its actions), gbl_rollout_at and, in
// collect_error / collect_policy_error, the collectors
inline const char *step_error(int64_t n, const void *state, const void *to_move, const void *done, const void *actions, int illegal_mode)
{
    GBL_N(n); GBL_PTR(state); GBL_PTR(to_move); GBL_PTR(done); GBL_PTR(actions);
    return illegal_mode_error(illegal_mode);
}

inline const char *rollout_error(int64_t n, const void *state, const void *to_move, const void *done, int illegal_mode)
{
    GBL_N(n); GBL_PTR(state); GBL_PTR(to_move); GBL_PTR(done);
    return illegal_mode_error(illegal_mode);
}

// (the device flavour looks at first_actions' alignment in front of these)
inline const char *collect_error(int64_t n, const void *first_actions, const void *first_status, const void *state, const void *to_move,
                                 const void *done, int illegal_mode, uint32_t plies, int64_t ply_stride, int64_t tile_stride)
{
    GBL_N(n);
    if (first_status && !first_actions) return "first_status without first_actions";
    if (const char *why = rollout_error(n, state, to_move, done, illegal_mode)) return why;
    return plies == 0 || strides_ok(n, plies, ply_stride, tile_stride) ? nullptr : kStridesMessage;
}

inline const char *collect_policy_error(int64_t n, const void *state, const void *to_move, const void *done, int illegal_mode, int policy0,
                                        int policy1, int opening_plies, bool has_turn, uint32_t plies, int64_t ply_stride, int64_t tile_stride)
{
    if (const char *why = rollout_error(n, state, to_move, done, illegal_mode)) return why;
    if (n == 0) return nullptr;
    if (policy0 < 0 || policy0 > 3 || policy1 < 0 || policy1 > 3) return "policy0 / policy1: GBL_POLICY_RANDOM, GBL_POLICY_GREEDY1, _GREEDY2 or _GREEDY3";
    if (opening_plies < 0) return "opening_plies < 0";
    if (opening_plies > 0 && !has_turn) return "opening_plies > 0 needs the per-board turn counter (turn must not be NULL)";
    return plies == 0 || strides_ok(n, plies, ply_stride, tile_stride) ? nullptr : kStridesMessage;
}

// gbl_greedy, and gbl_greedy_act_at, which also needs the history it appends to
inline const char *greedy_error(int64_t n, const void *state, const void *to_move, const void *action_out, int depth)
{
    GBL_N(n); GBL_PTR(state); GBL_PTR(to_move); GBL_PTR(action_out);
    return depth < 1 || depth > 3 ? "depth must be 1, 2 or 3" : nullptr;
}

inline const char *greedy_act_error(int64_t n, const void *state, const void *to_move, const void *hist, const void *action_out, int depth)
{
    GBL_N(n); GBL_PTR(state); GBL_PTR(to_move); GBL_PTR(hist);
    return greedy_error(n, state, to_move, action_out, depth);
}

inline const char *outcome_targets_error(int64_t n, const void *done_traj, const void *reward_traj, const void *mover_traj, const void *z_traj,
                                         uint32_t plies, int64_t ply_stride, int64_t tile_stride)
{
    GBL_N(n); GBL_PTR(done_traj); GBL_PTR(reward_traj); GBL_PTR(mover_traj); GBL_PTR(z_traj);
    if (plies > 32767u) return "plies must not exceed 32767";
    return plies == 0 || strides_ok(n, plies, ply_stride, tile_stride) ? nullptr : kStridesMessage;
}
#undef GBL_N
#undef GBL_PTR

// ---- board symmetries (include/gobblet_hip.h, "Board symmetries"): gbl_symmetry_apply and gbl_training_batch ------------------------
// One statement of the rule for the kernels and the host flavour.  Everything is in GATHER form -- "which input element lands in
// output element k" -- so that a lane that owns a whole row runs it with constant k (the divisions fold away) and a wavefront that
// fills a row cooperatively runs it with k = its lane.
constexpr int kSymmetries = 512;         // GBL_SYMMETRIES
constexpr int kBatchAttempts = 16;       // GBL_BATCH_ATTEMPTS
constexpr uint32_t kStreamBatch = 5u;    // generator stream of gbl_training_batch's draws

// sigma(p) from the header's (r, c) rule
__device__ __forceinline__ uint32_t sym_sigma(uint32_t s, uint32_t p)
{
    uint32_t r = p / 3u, c = p % 3u;
    c = (s & 4u) ? 2u - c : c;
#pragma unroll
    for (uint32_t i = 0; i < 3u; ++i) {
        const bool turn = i < (s & 3u);
        const uint32_t r2 = turn ? c : r, c2 = turn ? 2u - r : c;
        r = r2; c = c2;
    }
    return 3u * r + c;
}

// A decoded symmetry: sigma and its inverse as nine nibbles each (nibble p = the image of p), and the six swap bits
// (bit k: player_1's pair k, bit 3 + k: player_2's).
struct Sym {
    uint64_t fwd, inv;
    uint32_t swaps;
};

__device__ __forceinline__ Sym sym_of(uint32_t s)
{
    Sym S{0ull, 0ull, (s >> 3) & 63u};
#pragma unroll
    for (uint32_t p = 0; p < 9u; ++p) {
        const uint32_t q = sym_sigma(s, p);
        S.fwd |= (uint64_t)q << (4u * p);
        S.inv |= (uint64_t)p << (4u * q);
    }
    return S;
}

__device__ __forceinline__ uint32_t sym_pos(const Sym &S, uint32_t p) { return (uint32_t)(S.fwd >> (4u * p)) & 15u; }
__device__ __forceinline__ uint32_t sym_pos_inv(const Sym &S, uint32_t p) { return (uint32_t)(S.inv >> (4u * p)) & 15u; }
// tau_m on the piece INDEX i = piece - 1 in 0..5 (an involution: it is its own inverse)
__device__ __forceinline__ uint32_t sym_piece(const Sym &S, uint32_t m, uint32_t i) { return i ^ ((S.swaps >> (3u * m + (i >> 1))) & 1u); }

// A_m(a), a in [0, 54)
__device__ __forceinline__ uint32_t sym_action(const Sym &S, uint32_t m, uint32_t a) { return 9u * sym_piece(S, m, a / 9u) + sym_pos(S, a % 9u); }
// the action whose entry lands in entry k of an action-indexed row: A_m^-1(k)
__device__ __forceinline__ uint32_t sym_action_src(const Sym &S, uint32_t m, uint32_t k) { return 9u * sym_piece(S, m, k / 9u) + sym_pos_inv(S, k % 9u); }
// the observation byte that lands in byte k = 13 p + ch of agent m's observation row
__device__ __forceinline__ uint32_t sym_obs_src(const Sym &S, uint32_t m, uint32_t k)
{
    const uint32_t p = k / 13u, ch = k % 13u;
    const uint32_t from = ch < 6u ? sym_piece(S, m, ch) : ch < 12u ? 6u + sym_piece(S, m ^ 1u, ch - 6u) : 12u;
    return 13u * sym_pos_inv(S, p) + from;
}
// the state cell that lands in cell k = 9 l + p, and what becomes of its value
__device__ __forceinline__ uint32_t sym_state_src(const Sym &S, uint32_t k) { return 9u * (k / 9u) + sym_pos_inv(S, k % 9u); }
__device__ __forceinline__ int8_t sym_value(const Sym &S, int8_t v)
{
    const int a = v < 0 ? -v : v;
    if (a < 1 || a > 6) return v;
    const int t = (int)sym_piece(S, v < 0 ? 1u : 0u, (uint32_t)(a - 1)) + 1;
    return (int8_t)(v < 0 ? -t : t);
}

// Whole rows, for whoever owns one (a lane with its row in LDS; the host flavour with the row where it lives).  in != out.
__device__ __forceinline__ void sym_state_row(const int8_t *in, int8_t *out, const Sym &S)
{
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kCells; ++k) out[k] = sym_value(S, in[sym_state_src(S, k)]);
}
__device__ __forceinline__ void sym_obs_row(const int8_t *in, int8_t *out, const Sym &S, uint32_t m)
{
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kObs; ++k) out[k] = in[sym_obs_src(S, m, k)];
}
template <typename T>
__device__ __forceinline__ void sym_action_row(const T *in, T *out, const Sym &S, uint32_t m)
{
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kActions; ++k) out[k] = in[sym_action_src(S, m, k)];
}
__device__ __forceinline__ int32_t sym_action_any(const Sym &S, uint32_t m, int32_t a)
{
    return a >= 0 && a < kActions ? (int32_t)sym_action(S, m, (uint32_t)a) : a;
}

// gbl_training_batch: element (t, b) of a trajectory array, and attempt i of sample `id` (the header's draw rule)
__device__ __forceinline__ int64_t traj_cell(int64_t t, int64_t b, int64_t ply_stride, int64_t tile_stride)
{
    return t * ply_stride + (b >> 6) * tile_stride + (b & 63);
}
struct BatchDraw {
    uint32_t t, sym;
    int64_t b;
};
__device__ __forceinline__ BatchDraw batch_draw(uint64_t seed, uint64_t id, uint32_t call, uint32_t i, uint32_t plies, int64_t n)
{
    const Draw4 d = draw_block(seed, id, 4u * ((uint32_t)kBatchAttempts * call + i), kStreamBatch);
    return BatchDraw{1u + __umulhi(d.w[0], plies - 1u), d.w[2], (int64_t)(((uint64_t)d.w[1] * (uint64_t)n) >> 32)};
}
// is cell `at` = (t, b), whose predecessor (t - 1, b) is `prev`, a training sample?  (visits rows: 4-byte aligned on the device)
__device__ __forceinline__ bool batch_valid(const int8_t *z, const int8_t *done, const int16_t *visits, int64_t at, int64_t prev)
{
    if (z[at] == (int8_t)kZOpen || done[prev] != 0) return false;
    int sum = 0;
#ifndef GBL_HOST_EMU
    const uint32_t *v = reinterpret_cast<const uint32_t *>(visits + at * kActions);
#pragma unroll
    for (int k = 0; k < kActions / 2; ++k) {
        const uint32_t d = v[k];
        sum += (int)(int16_t)(d & 0xFFFFu) + (int)(int16_t)(d >> 16);
    }
#else
    for (int k = 0; k < kActions; ++k) sum += visits[at * kActions + k];
#endif
    return sum > 0;
}

// Argument checks of gbl_symmetry_apply, shared by both flavours (the device entry adds its alignment rules).  ok_zero: n == 0.
struct SymRowsArg {
    const void *in[6];  // state, obs, mask, visits, priors, actions
    void *out[6];
};
inline const char *symmetry_error(const void *sym, int sym_all, const void *agent, const SymRowsArg &R, int64_t n)
{
    static const char *const pair_msg[6] = {"state_in and state_out go together", "obs_in and obs_out go together",
                                            "mask_in and mask_out go together", "visits_in and visits_out go together",
                                            "priors_in and priors_out go together", "actions_in and actions_out go together"};
    static const char *const same_msg[6] = {"state_out must not be state_in: the transform is not in-place safe",
                                            "obs_out must not be obs_in: the transform is not in-place safe",
                                            "mask_out must not be mask_in: the transform is not in-place safe",
                                            "visits_out must not be visits_in: the transform is not in-place safe",
                                            "priors_out must not be priors_in: the transform is not in-place safe",
                                            "actions_out must not be actions_in: the transform is not in-place safe"};
    if (n < 0) return "n < 0";
    if (!sym && (sym_all < 0 || sym_all >= kSymmetries)) return "sym_all must be in [0, 512)";
    if (n == 0) return nullptr;
    bool needs_agent = false;
    for (int i = 0; i < 6; ++i) {
        if (!R.in[i] != !R.out[i]) return pair_msg[i];
        if (R.in[i] && R.in[i] == R.out[i]) return same_msg[i];
        needs_agent |= i > 0 && R.in[i];
    }
    if (needs_agent && !agent) return "agent must not be NULL when obs, an action-indexed row or actions are given";
    return nullptr;
}

// ... and of gbl_training_batch.
inline const char *batch_error(const void *obs_traj, const void *mask_traj, const void *visits_traj, const void *z_traj,
                               const void *done_traj, const void *mover_traj, int64_t n, uint32_t plies, int64_t ply_stride,
                               int64_t tile_stride, int64_t batch, int sym_mask, uint32_t call, const void *obs_out,
                               const void *mask_out, const void *index_out)
{
    if (plies < 2u || plies > 32767u) return "plies must be in [2, 32767]";
    if (batch < 0 || batch > ((int64_t)1 << 31)) return "batch must be in [0, 2^31]";
    if (sym_mask < 0 || sym_mask >= kSymmetries) return "sym_mask must be in [0, 511]";
    if (call >= (1u << 26)) return "call must be below 2^26";
    if (batch == 0) return nullptr;
    if (n < 1 || n > ((int64_t)1 << 31)) return "n must be in [1, 2^31]";
    if (!visits_traj) return "visits_traj must not be NULL";
    if (!z_traj) return "z_traj must not be NULL";
    if (!done_traj) return "done_traj must not be NULL";
    if (!mover_traj) return "mover_traj must not be NULL";
    if (!index_out) return "index_out must not be NULL";
    if (obs_out && !obs_traj) return "obs_out needs obs_traj";
    if (mask_out && !mask_traj) return "mask_out needs mask_traj";
    if (!strides_ok(n, plies, ply_stride, tile_stride)) return kStridesMessage;
    return nullptr;
}

// ---- replay buffer (include/gobblet_hip.h, "Replay buffer"): the rule's pieces, shared by the kernels and the host flavour ------------
constexpr int kReplayObsPitch = 128;    // GBL_REPLAY_OBS_PITCH (bytes)
constexpr int kReplayVisitsPitch = 64;  // GBL_REPLAY_VISITS_PITCH (int16 elements)
constexpr int kReplayMetaPitch = 64;    // GBL_REPLAY_META_PITCH (bytes)
constexpr int kReplayMetaZ = 54, kReplayMetaMover = 55, kReplayMetaTag = 56;  // GBL_REPLAY_META_*
constexpr uint32_t kStreamReplay = 7u;  // generator stream of gbl_replay_batch's draws
constexpr int64_t kReplayMaxCapacity = 0x7FFFFFFF;
constexpr int kReplayWsHead = 4;        // the workspace's first uint64s: T0, K, two of padding; then the chunks' ballots, then their bases

// chunk c = (t - 1) * tiles + tile holds the cells (t, 64 tile .. 64 tile + 63): ascending c, then ascending lane, is ascending (t, b)
inline int64_t replay_chunks(int64_t n, uint32_t plies) { return ((int64_t)plies - 1) * ((n + kTile - 1) / kTile); }
inline bool replay_window_ok(int64_t n, uint32_t plies) { return plies >= 2u && plies <= 32767u && n >= 1 && n <= ((int64_t)1 << 31); }
inline uint64_t replay_workspace_bytes(int64_t n, uint32_t plies)
{
    return replay_window_ok(n, plies) ? 8u * ((uint64_t)kReplayWsHead + 2u * (uint64_t)replay_chunks(n, plies)) : 0u;
}
// the cell of rank R of an append of K rows onto T0: is it written at all, and where
__device__ __forceinline__ bool replay_kept(uint64_t R, uint64_t K, uint64_t capacity) { return K - R <= capacity; }
__device__ __forceinline__ uint32_t replay_slot(uint64_t T0, uint64_t R, uint64_t capacity) { return (uint32_t)((T0 + R) % capacity); }

// sample `id` of gbl_replay_batch on a ring that has taken `total` rows: its slot (-1: the ring is empty) and its symmetry word
struct ReplayDraw {
    int64_t slot;
    uint32_t sym;
};
__device__ __forceinline__ ReplayDraw replay_draw(uint64_t seed, uint64_t id, uint32_t call, uint64_t total, uint64_t capacity, int64_t recent)
{
    const Draw4 d = draw_block(seed, id, 4u * ((uint32_t)kBatchAttempts * call), kStreamReplay);  // (batch_draw's attempt 0, another stream)
    const uint64_t live = total < capacity ? total : capacity;
    if (live == 0) return ReplayDraw{-1, 0u};
    const uint64_t span = recent > 0 && (uint64_t)recent < live ? (uint64_t)recent : live;
    const uint64_t age = __umulhi(d.w[0], (uint32_t)span), newest = (total - 1u) % capacity;
    return ReplayDraw{(int64_t)(newest >= age ? newest - age : newest + capacity - age), d.w[2]};
}

inline const char *replay_append_error(const void *obs_traj, const void *mask_traj, const void *visits_traj, const void *z_traj,
                                       const void *done_traj, const void *mover_traj, int64_t n, uint32_t plies, int64_t ply_stride,
                                       int64_t tile_stride, const void *ring_obs, const void *ring_visits, const void *ring_meta,
                                       int64_t capacity, const void *ring_state, const void *workspace, uint64_t workspace_bytes)
{
    if (plies < 2u || plies > 32767u) return "plies must be in [2, 32767]";
    if (n < 1 || n > ((int64_t)1 << 31)) return "n must be in [1, 2^31]";
    if (capacity < 1 || capacity > kReplayMaxCapacity) return "capacity must be in [1, 2^31 - 1]";
    if (!mask_traj) return "mask_traj must not be NULL";
    if (!visits_traj) return "visits_traj must not be NULL";
    if (!z_traj) return "z_traj must not be NULL";
    if (!done_traj) return "done_traj must not be NULL";
    if (!mover_traj) return "mover_traj must not be NULL";
    if (!ring_visits) return "ring_visits must not be NULL";
    if (!ring_meta) return "ring_meta must not be NULL";
    if (!ring_state) return "ring_state must not be NULL";
    if (!workspace) return "workspace must not be NULL";
    if (!ring_obs != !obs_traj) return "ring_obs and obs_traj go together";
    if (!strides_ok(n, plies, ply_stride, tile_stride)) return kStridesMessage;
    if (workspace_bytes < replay_workspace_bytes(n, plies)) return "workspace_bytes is below gbl_replay_workspace_bytes";
    return nullptr;
}

// (ok_zero: batch == 0 returns GBL_OK after the scalar checks)
inline const char *replay_batch_error(const void *ring_obs, const void *ring_visits, const void *ring_meta, int64_t capacity,
                                      const void *ring_state, int64_t recent, int64_t batch, int sym_mask, uint32_t call,
                                      const void *obs_out, const void *index_out)
{
    if (capacity < 1 || capacity > kReplayMaxCapacity) return "capacity must be in [1, 2^31 - 1]";
    if (batch < 0 || batch > ((int64_t)1 << 31)) return "batch must be in [0, 2^31]";
    if (sym_mask < 0 || sym_mask >= kSymmetries) return "sym_mask must be in [0, 511]";
    if (call >= (1u << 26)) return "call must be below 2^26";
    if (recent < 0) return "recent must not be negative";
    if (batch == 0) return nullptr;
    if (!ring_visits) return "ring_visits must not be NULL";
    if (!ring_meta) return "ring_meta must not be NULL";
    if (!ring_state) return "ring_state must not be NULL";
    if (!index_out) return "index_out must not be NULL";
    if (obs_out && !ring_obs) return "obs_out needs ring_obs";
    return nullptr;
}

// ---- prioritised replay (include/gobblet_hip.h, "Replay buffer", the priorities' paragraph) -----------------------------------------
// A leaf is 32 consecutive slots (one 128-byte line of ring_prio), a block 64 consecutive leaves (2 048 slots).  prio_index in uint64s:
//   [0] the ring_state[0] it was built for, [1] the weight of all live rows,
//   base[0 .. nblocks]   base[b] = the weight of the live slots of blocks 0 .. b - 1,
//   local[0 .. nleaves)  local[L] = the weight of the live slots of the leaves of L's block that lie before L.
// Two levels so that the build is two short launches: every block's local prefix by a workgroup of its own, then one scan over the blocks.
constexpr uint32_t kStreamReplayPrio = 8u;  // generator stream of gbl_replay_batch_prio's draws
constexpr int kReplayLeaf = 32, kReplayBlockLeaves = 64, kReplayPrioHead = 2;
constexpr uint64_t replay_prio_leaves(uint64_t capacity) { return (capacity + kReplayLeaf - 1) / kReplayLeaf; }
constexpr uint64_t replay_prio_blocks(uint64_t capacity) { return (replay_prio_leaves(capacity) + kReplayBlockLeaves - 1) / kReplayBlockLeaves; }
inline uint64_t replay_prio_index_bytes(int64_t capacity)
{
    if (capacity < 1 || capacity > kReplayMaxCapacity) return 0u;
    return 8u * (kReplayPrioHead + replay_prio_blocks((uint64_t)capacity) + 1u + replay_prio_leaves((uint64_t)capacity));
}
__device__ __forceinline__ uint64_t replay_weight(int32_t p) { return p > 0 ? (uint64_t)p : 0u; }
// floor(a b / 2^64) from the four 32 x 32 products (plain C++: the same text serves the kernels, the host flavour and the emulation)
__device__ __forceinline__ uint64_t replay_mulhi64(uint64_t a, uint64_t b)
{
    const uint64_t a0 = (uint32_t)a, a1 = a >> 32, b0 = (uint32_t)b, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (uint32_t)p01 + (uint32_t)p10;
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

struct ReplayPrioIndex {
    const uint64_t *base, *local;
    uint64_t leaves, blocks;
};
__device__ __forceinline__ ReplayPrioIndex replay_prio_view(const uint64_t *index, uint64_t capacity)
{
    const uint64_t blocks = replay_prio_blocks(capacity);
    return ReplayPrioIndex{index + kReplayPrioHead, index + kReplayPrioHead + blocks + 1u, replay_prio_leaves(capacity), blocks};
}

// the 32 entries of the leaf that starts at slot s as weights, 0 for slots that are not live: a whole leaf comes in as eight 16-byte
// vectors (independent loads: one trip to memory), the ragged last leaf of the array entry by entry
__device__ __forceinline__ void replay_leaf_weights(const int32_t *__restrict__ prio, uint64_t s, uint64_t capacity, uint64_t live, uint32_t w[kReplayLeaf])
{
    if (s + kReplayLeaf <= capacity) {
        const uint4 *v = reinterpret_cast<const uint4 *>(prio + s);
#pragma unroll
        for (int i = 0; i < kReplayLeaf / 4; ++i) {
            const uint4 p = v[i];
            w[4 * i] = p.x; w[4 * i + 1] = p.y; w[4 * i + 2] = p.z; w[4 * i + 3] = p.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kReplayLeaf; ++i) w[i] = s + i < capacity ? (uint32_t)prio[s + i] : 0u;
    }
#pragma unroll
    for (int i = 0; i < kReplayLeaf; ++i) w[i] = s + i < live ? (uint32_t)replay_weight((int32_t)w[i]) : 0u;
}

// the weight of the live slots below slot x (x <= capacity): the block's base, the leaf's local prefix and at most 31 entries of the leaf
__device__ __forceinline__ uint64_t replay_prio_prefix(const int32_t *__restrict__ prio, const ReplayPrioIndex &I, uint64_t x, uint64_t capacity,
                                                       uint64_t live)
{
    const uint64_t leaf = x / kReplayLeaf;
    if (leaf == I.leaves) return I.base[I.blocks];  // (x == capacity, a multiple of 32)
    uint64_t acc = I.base[leaf / kReplayBlockLeaves] + I.local[leaf];
    const uint32_t k = (uint32_t)(x % kReplayLeaf);
    if (k == 0) return acc;
    uint32_t w[kReplayLeaf];
    replay_leaf_weights(prio, leaf * kReplayLeaf, capacity, live, w);
#pragma unroll
    for (int i = 0; i < kReplayLeaf - 1; ++i) acc += (uint32_t)i < k ? w[i] : 0u;
    return acc;
}

// what is the same for every sample of a launch: the span, its weight W (0: every sample fails), and where the span's order starts in
// the ring's prefix -- the span is the slots [first, capacity) and then [0, ...) when it crosses the ring's end: the prefix value `base` of
// its first slot and the weight `head` of its first range (W when it does not cross).
struct ReplayPrioSpan {
    uint64_t live, span, W, base, head;
};
__device__ __forceinline__ ReplayPrioSpan replay_prio_span(const int32_t *__restrict__ prio, const uint64_t *__restrict__ index, uint64_t total,
                                                           uint64_t capacity, int64_t recent)
{
    const uint64_t live = total < capacity ? total : capacity;
    const uint64_t span = recent > 0 && (uint64_t)recent < live ? (uint64_t)recent : live;
    ReplayPrioSpan P{live, span, 0u, 0u, 0u};
    if (live == 0 || index[0] != total) return P;
    const ReplayPrioIndex I = replay_prio_view(index, capacity);
    if (span == live) {  // (every live row: the build left the sum)
        P.W = index[1];
        const uint64_t first = total < capacity ? 0u : total % capacity;
        P.base = first ? replay_prio_prefix(prio, I, first, capacity, live) : 0u;
        P.head = P.W - P.base;
        return P;
    }
    const uint64_t first = (total - span) % capacity;
    P.base = replay_prio_prefix(prio, I, first, capacity, live);
    if (first + span <= capacity) {
        P.head = P.W = replay_prio_prefix(prio, I, first + span, capacity, live) - P.base;
    } else {
        P.head = index[1] - P.base;  // (the ring has wrapped: the first range runs to the ring's end)
        P.W = P.head + replay_prio_prefix(prio, I, first + span - capacity, capacity, live);
    }
    return P;
}

// sample `id` of gbl_replay_batch_prio: the slot (-1: a failed sample), its weight and its symmetry word.  With a fresh index the target is
// below the ring's whole weight and the walk ends inside the leaf; with a stale one the slot is still inside [0, capacity).
struct ReplayPrioDraw {
    int64_t slot;
    uint32_t weight, sym;
};
__device__ __forceinline__ ReplayPrioDraw replay_prio_draw(uint64_t seed, uint64_t id, uint32_t call, const ReplayPrioSpan &P, uint64_t capacity,
                                                           const int32_t *__restrict__ prio, const uint64_t *__restrict__ index)
{
    const Draw4 d = draw_block(seed, id, 4u * ((uint32_t)kBatchAttempts * call), kStreamReplayPrio);
    if (P.W == 0) return ReplayPrioDraw{-1, 0u, 0u};
    const uint64_t r = replay_mulhi64(((uint64_t)d.w[0] << 32) | d.w[1], P.W);
    const uint64_t target = r < P.head ? P.base + r : r - P.head;  // (in the ring's own prefix: the slot is the first whose prefix passes it)
    const ReplayPrioIndex I = replay_prio_view(index, capacity);
    uint64_t lo = 0, hi = I.blocks;  // the last block whose base does not pass the target ...
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (I.base[mid] <= target) lo = mid; else hi = mid;
    }
    const uint64_t in_block = target - I.base[lo];
    hi = (lo + 1u) * kReplayBlockLeaves < I.leaves ? (lo + 1u) * kReplayBlockLeaves : I.leaves;
    lo *= kReplayBlockLeaves;  // ... and in it the last leaf whose local prefix does not
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (I.local[mid] <= in_block) lo = mid; else hi = mid;
    }
    const uint64_t s = lo * kReplayLeaf, in_leaf = in_block - I.local[lo];
    uint32_t w[kReplayLeaf];
    replay_leaf_weights(prio, s, capacity, P.live, w);
    uint64_t acc = 0;
    uint32_t at = 0, weight = w[0];  // (a stale index may pass no entry: the leaf's first slot, inside [0, capacity))
    bool found = false;
#pragma unroll
    for (int i = 0; i < kReplayLeaf; ++i) {
        acc += w[i];
        if (!found && acc > in_leaf) { found = true; at = (uint32_t)i; weight = w[i]; }
    }
    return ReplayPrioDraw{(int64_t)(s + at), weight, d.w[2]};
}

inline const char *replay_prio_append_error(const void *visits_traj, const void *z_traj, const void *done_traj, int64_t n, uint32_t plies,
                                            int64_t ply_stride, int64_t tile_stride, const void *ring_prio, int64_t capacity,
                                            const void *ring_state, const void *workspace, uint64_t workspace_bytes)
{
    if (plies < 2u || plies > 32767u) return "plies must be in [2, 32767]";
    if (n < 1 || n > ((int64_t)1 << 31)) return "n must be in [1, 2^31]";
    if (capacity < 1 || capacity > kReplayMaxCapacity) return "capacity must be in [1, 2^31 - 1]";
    if (!visits_traj) return "visits_traj must not be NULL";
    if (!z_traj) return "z_traj must not be NULL";
    if (!done_traj) return "done_traj must not be NULL";
    if (!ring_prio) return "ring_prio must not be NULL";
    if (!ring_state) return "ring_state must not be NULL";
    if (!workspace) return "workspace must not be NULL";
    if (!strides_ok(n, plies, ply_stride, tile_stride)) return kStridesMessage;
    if (workspace_bytes < replay_workspace_bytes(n, plies)) return "workspace_bytes is below gbl_replay_workspace_bytes";
    return nullptr;
}

// (batch == 0 returns GBL_OK after the scalar checks)
inline const char *replay_prio_update_error(const void *index, const void *values, int64_t batch, const void *ring_prio, int64_t capacity)
{
    if (capacity < 1 || capacity > kReplayMaxCapacity) return "capacity must be in [1, 2^31 - 1]";
    if (batch < 0 || batch > ((int64_t)1 << 31)) return "batch must be in [0, 2^31]";
    if (batch == 0) return nullptr;
    if (!index) return "index must not be NULL";
    if (!values) return "values must not be NULL";
    if (!ring_prio) return "ring_prio must not be NULL";
    return nullptr;
}

inline const char *replay_prio_index_error(const void *ring_prio, int64_t capacity, const void *ring_state, const void *prio_index,
                                           uint64_t index_bytes)
{
    if (capacity < 1 || capacity > kReplayMaxCapacity) return "capacity must be in [1, 2^31 - 1]";
    if (!ring_prio) return "ring_prio must not be NULL";
    if (!ring_state) return "ring_state must not be NULL";
    if (!prio_index) return "prio_index must not be NULL";
    if (index_bytes < replay_prio_index_bytes(capacity)) return "index_bytes is below gbl_replay_prio_index_bytes";
    return nullptr;
}

// gbl_replay_batch's checks, and with batch > 0 the two blocks of the priorities
inline const char *replay_batch_prio_error(const void *ring_obs, const void *ring_visits, const void *ring_meta, int64_t capacity,
                                           const void *ring_state, const void *ring_prio, const void *prio_index, int64_t recent, int64_t batch,
                                           int sym_mask, uint32_t call, const void *obs_out, const void *index_out)
{
    if (const char *why = replay_batch_error(ring_obs, ring_visits, ring_meta, capacity, ring_state, recent, batch, sym_mask, call, obs_out, index_out))
        return why;
    if (batch == 0) return nullptr;
    if (!ring_prio) return "ring_prio must not be NULL";
    if (!prio_index) return "prio_index must not be NULL";
    return nullptr;
}

// ---- tablebase (include/gobblet_hip.h, "Exact tablebase"): the rule's pieces, shared by the kernels and the host flavour ---------------
// A position is two 27-bit cell sets, the mover's (`own`) and the other side's (`oth`), level k in bits 9k .. 9k + 8.  Its index comes
// from three table look-ups (one per level: the rank of the level's ternary number), its successors from bit arithmetic on the
// two sets; only the level a piece moves on changes its code, so a successor's index costs ONE look-up.
constexpr int kTbTerminal = -128;       // GBL_TB_TERMINAL
constexpr int kTbMaxSweep = 126;        // GBL_TB_MAX_SWEEP
constexpr uint32_t kTbTernary = 19683;  // 3^9 level configurations
constexpr uint32_t kTbLevels2 = 1423, kTbLevels1 = 91;
// `aux` in bytes: rank2 uint16[19683] | inv2 uint16[1423] | inv1 uint16[91] | tern uint16[512] | rank1 uint8[19683], each on a 4-byte boundary
constexpr uint32_t kTbAuxRank2 = 0, kTbAuxInv2 = 39368, kTbAuxInv1 = 42216, kTbAuxTern = 42400, kTbAuxRank1 = 43424;
constexpr uint32_t kTbAuxBytes = 63120;  // GBL_TB_AUX_BYTES
constexpr uint32_t kTbNoRank = 0xFFFFFFFFu;

struct TbAux {
    const uint16_t *rank2, *inv2, *inv1, *tern;
    const uint8_t *rank1;
};
__device__ __forceinline__ TbAux tb_aux(const void *base)
{
    const uint8_t *b = static_cast<const uint8_t *>(base);
    return TbAux{reinterpret_cast<const uint16_t *>(b + kTbAuxRank2), reinterpret_cast<const uint16_t *>(b + kTbAuxInv2),
                 reinterpret_cast<const uint16_t *>(b + kTbAuxInv1), reinterpret_cast<const uint16_t *>(b + kTbAuxTern), b + kTbAuxRank1};
}

// the inventory as the kernels take it: c_k, L_k and the index strides (all below 2^32: 1 423^3 = 2 881 473 967)
struct TbShape {
    uint32_t c[3], L[3];
    uint64_t positions;
};
inline uint32_t tb_levels(int c) { return c == 0 ? 1u : (c == 1 ? kTbLevels1 : kTbLevels2); }
inline TbShape tb_shape(const int32_t *inventory)
{
    TbShape S;
    for (int k = 0; k < 3; ++k) {
        S.c[k] = (uint32_t)inventory[k];
        S.L[k] = tb_levels(inventory[k]);
    }
    S.positions = (uint64_t)S.L[0] * S.L[1] * S.L[2];
    return S;
}

// what a ternary level number is worth to the two rank tables: bit 0 = admissible for c = 2, bit 16 = for c = 1 (packed for the scan)
__device__ __forceinline__ uint32_t tb_admissible(uint32_t t)
{
    uint32_t n1 = 0, n2 = 0;
#pragma unroll
    for (int pos = 0; pos < 9; ++pos) {
        const uint32_t d = t % 3u;
        t /= 3u;
        n1 += d == 1u;
        n2 += d == 2u;
    }
    return (uint32_t)(n1 <= 2u && n2 <= 2u) | ((uint32_t)(n1 <= 1u && n2 <= 1u) << 16);
}
__device__ __forceinline__ uint32_t tb_tern_of(uint32_t cells)  // sum of 3^pos over a 9-bit cell set
{
    uint32_t t = 0, w = 1;
#pragma unroll
    for (int pos = 0; pos < 9; ++pos, w *= 3u) t += ((cells >> pos) & 1u) * w;
    return t;
}

// code of one level (kTbNoRank: more cells of a colour than c) and back
__device__ __forceinline__ uint32_t tb_code(const TbAux &A, uint32_t c, uint32_t own9, uint32_t oth9)
{
    const uint32_t t = (uint32_t)A.tern[own9] + 2u * (uint32_t)A.tern[oth9];
    if (c == 2u) {
        const uint32_t r = A.rank2[t];
        return r == 0xFFFFu ? kTbNoRank : r;
    }
    if (c == 1u) {
        const uint32_t r = A.rank1[t];
        return r == 0xFFu ? kTbNoRank : r;
    }
    return t == 0u ? 0u : kTbNoRank;
}
struct TbPos {
    uint32_t own, oth;
};
__device__ __forceinline__ void tb_level_cells(const TbAux &A, uint32_t c, uint32_t code, int level, TbPos &p)
{
    uint32_t t = c == 2u ? A.inv2[code] : (c == 1u ? A.inv1[code] : 0u);
#pragma unroll
    for (int pos = 0; pos < 9; ++pos) {
        const uint32_t d = t % 3u;
        t /= 3u;
        p.own |= (uint32_t)(d == 1u) << (9 * level + pos);
        p.oth |= (uint32_t)(d == 2u) << (9 * level + pos);
    }
}
__device__ __forceinline__ TbPos tb_position_of(const TbAux &A, const TbShape &S, uint32_t index)
{
    TbPos p{0u, 0u};
    const uint32_t upper = index / S.L[0];
    tb_level_cells(A, S.c[0], index - upper * S.L[0], 0, p);
    const uint32_t top = upper / S.L[1];
    tb_level_cells(A, S.c[1], upper - top * S.L[1], 1, p);
    tb_level_cells(A, S.c[2], top, 2, p);
    return p;
}
// the index of (own, oth), or -1
__device__ __forceinline__ int64_t tb_index_of(const TbAux &A, const TbShape &S, const TbPos &p)
{
    const uint32_t c0 = tb_code(A, S.c[0], p.own & 0x1FFu, p.oth & 0x1FFu), c1 = tb_code(A, S.c[1], (p.own >> 9) & 0x1FFu, (p.oth >> 9) & 0x1FFu),
                   c2 = tb_code(A, S.c[2], (p.own >> 18) & 0x1FFu, (p.oth >> 18) & 0x1FFu);
    if ((c0 | c1 | c2) == kTbNoRank) return -1;  // (a code is below 1 423: only kTbNoRank sets every bit)
    return (int64_t)(((uint64_t)c2 * S.L[1] + c1) * S.L[0] + c0);
}
// check_for_winner() of (own, oth): +1 the mover's colour, -1 the other, 0 no line (a line cannot match both colours)
__device__ __forceinline__ int tb_winner(uint32_t own, uint32_t oth)
{
    return winner_from_matches(line_matches_of(own, own | oth), line_matches_of(oth, own | oth));
}

// the header's rank on results up to +-126, as an order key: 1 .. 255, 0 = no move yet (reads back as V = 0)
__device__ __forceinline__ uint32_t tb_key(int c) { return (uint32_t)((c > 0 ? 128 - c : (c < 0 ? -128 - c : 0)) + 128); }
__device__ __forceinline__ int tb_of_key(uint32_t key)
{
    const int r = (int)key - 128;
    return key == 0u ? 0 : (r > 0 ? 128 - r : (r < 0 ? -128 - r : 0));
}
__device__ __forceinline__ uint32_t tb_action_key(int c, uint32_t a) { return (tb_key(c) << 6) | (63u - a); }
__device__ __forceinline__ int tb_action_of(uint32_t best) { return best ? 63 - (int)(best & 63u) : -1; }
__device__ __forceinline__ int tb_value_of(uint32_t best) { return tb_of_key(best >> 6); }
// c(a) from the byte u of the position after a; `proven`: the largest |u| that counts (k - 1 in sweep k, 127 in a probe)
__device__ __forceinline__ int tb_parent(int u, int proven)
{
    const int au = u < 0 ? -u : u;
    return au >= 1 && au <= proven ? solve_parent(u) : 0;  // (GBL_TB_TERMINAL reads 128: never proven)
}

// Sweep k >= 1 at one position whose byte is still 0: V as the header defines it.  The moves: level after level, source after source
// (bit 9 of `from` = the reserve), destination after destination.  A c(a) == k > 0 ends the walk: on the table of sweeps 0 .. k - 1
// nothing of this position ranks above +k (a +j, j < k, would have been written in sweep j).
__device__ __forceinline__ int tb_sweep_value(const TbAux &A, const TbShape &S, const TbPos &p, int k, const int8_t *table)
{
    const uint32_t stride[3] = {1u, S.L[0], S.L[0] * S.L[1]};
    uint32_t swapped[3], total = 0;  // the level codes as the other side sees them
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        swapped[l] = tb_code(A, S.c[l], (p.oth >> (9 * l)) & 0x1FFu, (p.own >> (9 * l)) & 0x1FFu) * stride[l];
        total += swapped[l];
    }
    const uint32_t occ = p.own | p.oth;
    uint32_t best = 0;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        if (S.c[l] == 0u) continue;
        uint32_t above = 0;
#pragma unroll
        for (int j = l + 1; j < 3; ++j) above |= (occ >> (9 * j)) & 0x1FFu;
        const uint32_t own_l = (p.own >> (9 * l)) & 0x1FFu;
        const uint32_t dest = ~(above | (occ >> (9 * l))) & 0x1FFu;
        if (!dest) continue;
        const uint32_t from = (own_l & ~above) | ((uint32_t)__popc(own_l) < S.c[l] ? 0x200u : 0u);
        const uint32_t base = total - swapped[l], oth_tern = A.tern[(p.oth >> (9 * l)) & 0x1FFu];
        for (uint32_t f = from; f; f &= f - 1u) {
            const uint32_t kept = own_l & ~(f & (0u - f));  // (the reserve's bit 9 clears nothing)
            for (uint32_t d = dest; d; d &= d - 1u) {
                const uint32_t now = kept | (d & (0u - d));
                const int w = tb_winner((p.own & ~(0x1FFu << (9 * l))) | (now << (9 * l)), p.oth);
                int c = w;
                if (w == 0 && k > 1) {
                    const uint32_t t = oth_tern + 2u * (uint32_t)A.tern[now];  // the level as the other side sees it: admissible by construction
                    const uint32_t code = S.c[l] == 2u ? (uint32_t)A.rank2[t] : (uint32_t)A.rank1[t];
                    c = tb_parent(table[base + code * stride[l]], k - 1);
                }
                if (c > 0 && c == k) return k;
                const uint32_t key = tb_key(c);
                best = key > best ? key : best;
            }
        }
    }
    return tb_of_key(best);
}

// a concrete board's planes as `viewer` (0 / 1) sees them, and whether it is a state of the inventory (only pieces that exist)
__device__ __forceinline__ TbPos tb_view(const Planes &p, int viewer)
{
    const uint32_t pos = p.nz & ~p.neg & 0x7FFFFFFu, neg = p.nz & p.neg & 0x7FFFFFFu;
    return viewer ? TbPos{neg, pos} : TbPos{pos, neg};
}
__device__ __forceinline__ bool tb_pieces_exist(const Planes &p, const TbShape &S)
{
    bool ok = true;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const uint32_t cells = (p.nz >> (9 * l)) & 0x1FFu, even = cells & ~(p.odd >> (9 * l));  // (piece 2l + 2 is the even one)
        ok = ok && (S.c[l] == 2u || (S.c[l] == 1u ? even == 0u : cells == 0u));
    }
    return ok;
}
__device__ __forceinline__ int64_t tb_board_index(const TbAux &A, const TbShape &S, const Planes &p, int viewer)
{
    return tb_pieces_exist(p, S) ? tb_index_of(A, S, tb_view(p, viewer)) : -1;
}
// the actions of the pieces the inventory has: piece number 2l + 1 + j exists for j < c_l
__device__ __forceinline__ uint64_t tb_piece_actions(const TbShape &S)
{
    uint64_t m = 0;
#pragma unroll
    for (int l = 0; l < 3; ++l)
        for (uint32_t j = 0; j < S.c[l]; ++j) m |= 0x1FFull << (9u * (2u * (uint32_t)l + j));
    return m;
}
// the probe's c(a) for a candidate a of `mover` on the concrete board p (a state of the inventory)
__device__ __forceinline__ int tb_probe_action(const TbAux &A, const TbShape &S, const int8_t *table, const Planes &p, int mover, uint32_t a)
{
    Planes q = p;
    move_planes(q, mover, a);
    const int now = solve_now(winner_of(q), mover);
    if (now != 0) return now;
    const int64_t child = tb_index_of(A, S, tb_view(q, mover ^ 1));
    return child < 0 ? 0 : tb_parent(table[child], 127);
}
// position `index` as a contract row with player_1 to move: own cells positive, the lowest piece number on the lowest cell
__device__ __forceinline__ void tb_row_of(const TbAux &A, const TbShape &S, int64_t index, int8_t *row)
{
    if (index < 0 || (uint64_t)index >= S.positions) {
        for (int i = 0; i < kCells; ++i) row[i] = (int8_t)kTbTerminal;
        return;
    }
    const TbPos p = tb_position_of(A, S, (uint32_t)index);
    for (int l = 0; l < 3; ++l) {
        int own = 0, oth = 0;
        for (int pos = 0; pos < 9; ++pos) {
            const int cell = 9 * l + pos;
            row[cell] = ((p.own >> cell) & 1u) ? (int8_t)(2 * l + 1 + own++) : (((p.oth >> cell) & 1u) ? (int8_t)-(2 * l + 1 + oth++) : (int8_t)0);
        }
    }
}

// Each *_error returns the message of the first rule the arguments break, or nullptr (all GBL_ERR_ARG; the device flavour's alignment
// rules follow there)
inline const char *tb_sweep_error(const int32_t *inventory, const void *aux, const void *table, const void *out, int64_t first, int64_t count,
                                  int k, const void *decided)
{
    if (const char *why = tb_inventory_error(inventory)) return why;
    if (k < 0 || k > kTbMaxSweep) return "k must be in [0, 126]";
    const uint64_t positions = tb_shape(inventory).positions;
    if (first < 0 || count < 0 || (uint64_t)first > positions || (uint64_t)count > positions - (uint64_t)first)
        return "first / count must lie inside the universe";
    if (count == 0) return nullptr;
    if (!aux) return "aux must not be NULL";
    if (!out) return "out must not be NULL";
    if (!decided) return "decided must not be NULL";
    if (k >= 2 && !table) return "table must not be NULL for k >= 2";
    return nullptr;
}
// (n == 0 passes whatever the pointers are: the caller returns GBL_OK before using them)
inline const char *tb_rows_error(const int32_t *inventory, const void *aux, int64_t n, const void *a, const char *a_msg, const void *b,
                                 const char *b_msg, const void *c, const char *c_msg)
{
    if (const char *why = tb_inventory_error(inventory)) return why;
    if (n < 0) return "n < 0";
    if (n == 0) return nullptr;
    if (!aux) return "aux must not be NULL";
    if (!a) return a_msg;
    if (!b) return b_msg;
    if (!c) return c_msg;
    return nullptr;
}

// ---- tablebase targets (include/gobblet_hip.h, "Tablebase targets"): the scalar pieces of the rule, shared by k_tb_targets and the host flavour
__device__ __forceinline__ int tb_sign(int c) { return (c > 0) - (c < 0); }
// whether a candidate's result BYTE c (the probe's outcome byte) belongs to the set O of a row of value `value`: R (mode 0, the result
// kept) or S (mode 1, c == value).  A c(a) of +-128 -- from a table byte of +-127, which no sweep writes -- reads GBL_SOLVE_NONE as a byte
// (its order key is a draw's either way): such a candidate counts for the probe's value and action and belongs to neither set.
__device__ __forceinline__ bool tb_target_keeps(int c, int value, int mode)
{
    return c != kSolveNone && (mode == kTbTargetShortest ? c == value : tb_sign(c) == tb_sign(value));
}
// a TABLEBASE mover's ply in gbl_collect_search_tb: its value from the probe's V and the sum of its visits row (count on every action of O)
__device__ __forceinline__ int tb_play_value(int value, int sum) { return tb_sign(value) * 128 * sum; }
// the order key of an old visit count (0: not positive); the largest key is the argmax, the lowest index on ties
__device__ __forceinline__ uint32_t tb_visit_key(int v, uint32_t a) { return v > 0 ? ((uint32_t)v << 6) | (63u - a) : 0u; }
// a labelled row's census byte: `top` the largest tb_visit_key of the old visits (0 without visits_in), `keeps` the set R as bits
__device__ __forceinline__ int tb_census(uint32_t top, uint64_t keeps, bool has_z, int z_old, int z_new)
{
    const int kept = top ? (int)((keeps >> (63u - (top & 63u))) & 1ull) : 4;
    return kept | (has_z && z_old == z_new ? 2 : 0);
}

// one pitched array of a gbl_tb_targets call, in bytes: rows of `row` bytes, `pitch` bytes apart
struct TbSpan {
    uintptr_t base;
    uint64_t pitch, row;
};
inline TbSpan tb_span(const void *p, int64_t pitch, int64_t row, int64_t elem)
{
    return TbSpan{reinterpret_cast<uintptr_t>(p), (uint64_t)(pitch * elem), (uint64_t)(row * elem)};
}
// whether two arrays of n rows share a byte.  Arrays whose extents intersect must have one byte pitch (then the rows interleave, as
// z does with the mask in ring_meta, and the test is exact); with two pitches an intersection of the extents counts as an overlap.
inline bool tb_spans_overlap(const TbSpan &a, const TbSpan &b, int64_t n)
{
    if (!a.base || !b.base) return false;
    const uint64_t ea = (uint64_t)(n - 1) * a.pitch + a.row, eb = (uint64_t)(n - 1) * b.pitch + b.row;
    if (a.base + ea <= b.base || b.base + eb <= a.base) return false;
    if (n == 1) return true;
    if (a.pitch != b.pitch) return true;
    const uint64_t d = b.base >= a.base ? (b.base - a.base) % a.pitch : (a.pitch - (a.base - b.base) % a.pitch) % a.pitch;
    return d < a.row || d + b.row > a.pitch;
}

// the message of the first rule a gbl_tb_targets call breaks, or nullptr; *empty = the call has nothing to do (n == 0 after the scalar checks)
inline const char *tb_targets_error(const int32_t *inventory, const void *aux, const void *table, const void *obs, int64_t obs_pitch,
                                    const void *mask, int64_t mask_pitch, const void *visits_in, const void *visits_out, int64_t visits_pitch,
                                    const void *z_in, const void *z_out, int64_t z_pitch, int mode, int count, const void *value_out,
                                    const void *outcome_out, const void *census_out, int64_t n, bool *empty)
{
    *empty = false;
    if (const char *why = tb_inventory_error(inventory)) return why;
    if (n < 0) return "n < 0";
    if (mode != kTbTargetResult && mode != kTbTargetShortest) return "mode must be GBL_TB_TARGET_RESULT or GBL_TB_TARGET_SHORTEST";
    if (count < 1 || count > kTbTargetMaxCount) return "count must be in [1, 600]";
    if (obs_pitch < kObs) return "obs_pitch must be at least 117";
    if (mask && mask_pitch < kActions) return "mask_pitch must be at least 54";
    if ((visits_in || visits_out) && visits_pitch < kActions) return "visits_pitch must be at least 54";
    if (z_pitch < 1) return "z_pitch must be at least 1";
    if (n == 0) {
        *empty = true;
        return nullptr;
    }
    if (!aux) return "aux must not be NULL";
    if (!table) return "table must not be NULL";
    if (!obs) return "obs must not be NULL";
    if (!z_out) return "z_out must not be NULL";
    // every output against every input; visits_in == visits_out and z_in == z_out are the in-place forms
    const TbSpan in[6] = {tb_span(obs, obs_pitch, kObs, 1), tb_span(mask, mask_pitch, kActions, 1),
                          tb_span(visits_in == visits_out ? nullptr : visits_in, visits_pitch, kActions, 2),
                          tb_span(z_in == z_out ? nullptr : z_in, z_pitch, 1, 1),
                          tb_span(aux, 0, kTbAuxBytes, 1), tb_span(table, 0, (int64_t)tb_shape(inventory).positions, 1)};
    const TbSpan out[5] = {tb_span(visits_out, visits_pitch, kActions, 2), tb_span(z_out, z_pitch, 1, 1), tb_span(value_out, 1, 1, 1),
                           tb_span(outcome_out, kActions, kActions, 1), tb_span(census_out, 1, 1, 1)};
    for (int o = 0; o < 5; ++o)
        for (int i = 0; i < 6; ++i) {
            // (aux and table are single rows whatever n is; an in-place pair is still checked against the other inputs)
            const bool one = i >= 4;
            if (one ? tb_spans_overlap(TbSpan{out[o].base, 0, (uint64_t)(n - 1) * out[o].pitch + out[o].row}, in[i], 1)
                    : tb_spans_overlap(in[i], out[o], n))
                return "an output overlaps an input (only visits_in == visits_out and z_in == z_out may alias)";
        }
    return nullptr;
}

// ---- reanalysis (include/gobblet_hip.h, "Reanalysis"): the scalar pieces of the rule, shared by k_reanalyse and the host flavour ------
// the drift of a row with a candidate: diff = sum over a of |o_a Sn - n_a So| (at most 2 So Sn <= 2 * 54 * 32767 * 512 < 2^32, so the
// sum and the divisor fit 32 bits and the product by 1024 fits 64); has_old: visits_in is given
__device__ __forceinline__ int reanalyse_drift(bool has_old, uint32_t So, uint32_t Sn, uint32_t diff)
{
    if (!has_old) return -1;
    if (!So) return 1024;
    return (int)((1024ull * (uint64_t)diff) / (2ull * (uint64_t)So * (uint64_t)Sn));
}
// gbl_reanalyse_gumbel's drift: the same quotient over the target bytes, Sn <= 54 * 255 -- single terms still fit 32 bits (at most
// 32767 * 13770), their sum (at most 2 So Sn, about 4.9e10) does not: diff and the divisor are 64-bit, the product by 1024 (5e13) fits
__device__ __forceinline__ int reanalyse_drift64(bool has_old, uint32_t So, uint32_t Sn, uint64_t diff)
{
    if (!has_old) return -1;
    if (!So) return 1024;
    return (int)((1024ull * diff) / (2ull * (uint64_t)So * (uint64_t)Sn));
}
// the census byte of a row with a candidate: `top_old` / `top_new` the largest tb_visit_key of the old visits (0: none positive, or no
// visits_in) and of the new ones (never 0: every iteration visits a child of the root); tb_census with the new argmax as the only kept action
__device__ __forceinline__ int reanalyse_census(uint32_t top_old, uint32_t top_new, bool has_z, int z_old, int root_q)
{
    return tb_census(top_old, 1ull << (63u - (top_new & 63u)), has_z, z_old, tb_sign(root_q));
}

// the message of the first rule a gbl_reanalyse call breaks, or nullptr; *empty = the call has nothing to do (n == 0 after the scalar checks).
// gum: gbl_reanalyse_gumbel's own arguments (nullptr: gbl_reanalyse) -- call in front of n < 0, the board ids and the rule's four behind
// it, and gumbel_out among the outputs.
struct ReanalyseGumbelCheck {
    int considered, gumbel_noise, visit_offset, scale;
    uint64_t env_base;
    uint32_t call;
    const void *gumbel_out;
};
template <typename Ev>
inline const char *reanalyse_error(const Ev *ev, int iterations, int explore, const void *obs, int64_t obs_pitch, const void *mask,
                                   int64_t mask_pitch, const void *visits_in, const void *visits_out, int64_t visits_pitch, const void *z_in,
                                   int64_t z_pitch, const void *root_value_out, const void *root_priors_out, const void *action_out,
                                   const void *nodes_out, const void *drift_out, const void *census_out, int64_t n, bool *empty,
                                   const ReanalyseGumbelCheck *gum = nullptr)
{
    *empty = false;
    const void *gumbel_out = gum ? gum->gumbel_out : nullptr;
    if (const char *why = evaluator_error(ev)) return why;
    if (const char *why = tree_eval_budget_error(iterations, explore)) return why;
    if (gum && gum->call >= (1u << 24)) return "call must be below 2^24";
    if (n < 0) return "n < 0";
    if (gum) {
        if (const char *why = env_range_error(gum->env_base, n)) return why;
        if (const char *why = gumbel_error(gum->considered, gum->gumbel_noise, gum->visit_offset, gum->scale)) return why;
    }
    if (obs_pitch < kObs) return "obs_pitch must be at least 117";
    if (mask && mask_pitch < kActions) return "mask_pitch must be at least 54";
    if ((visits_in || visits_out) && visits_pitch < kActions) return "visits_pitch must be at least 54";
    if (z_in && z_pitch < 1) return "z_pitch must be at least 1";
    if (n == 0) {
        *empty = true;
        return nullptr;
    }
    if (const char *why = evaluator_pointers_error(ev)) return why;
    if (!obs) return "obs must not be NULL";
    if (!visits_out && !root_value_out && !root_priors_out && !action_out && !nodes_out && !drift_out && !census_out && !gumbel_out)
        return "at least one output must be given";
    // every output against every input; visits_in == visits_out is the in-place form (that one pair is let through: the other outputs
    // are still checked against visits_in).  The evaluator's arrays are single rows.
    const int64_t H = ev->hidden;
    const TbSpan in[8] = {tb_span(obs, obs_pitch, kObs, 1), tb_span(mask, mask_pitch, kActions, 1),
                          tb_span(visits_in, visits_pitch, kActions, 2), tb_span(z_in, z_pitch, 1, 1),
                          tb_span(ev->w1, 0, (int64_t)kObs * H, 1), tb_span(ev->b1, 0, H, 4), tb_span(ev->w2, 0, H * kEvalOutputs, 1),
                          tb_span(ev->b2, 0, kEvalOutputs, 4)};
    const TbSpan out[8] = {tb_span(visits_out, visits_pitch, kActions, 2), tb_span(root_value_out, 1, 1, 4),
                           tb_span(root_priors_out, kActions, kActions, 1), tb_span(action_out, 1, 1, 4), tb_span(nodes_out, 1, 1, 4),
                           tb_span(drift_out, 1, 1, 4), tb_span(census_out, 1, 1, 1), tb_span(gumbel_out, kActions, kActions, 2)};
    for (int o = 0; o < 8; ++o)
        for (int i = 0; i < 8; ++i) {
            if (o == 0 && i == 2 && visits_in == visits_out) continue;
            const bool one = i >= 4;
            if (one ? tb_spans_overlap(TbSpan{out[o].base, 0, (uint64_t)(n - 1) * out[o].pitch + out[o].row}, in[i], 1)
                    : tb_spans_overlap(in[i], out[o], n))
                return "an output overlaps an input (only visits_in == visits_out may alias)";
        }
    return nullptr;
}

// ---- gbl_train_step (include/gobblet_hip.h, "One Adam step of the FLOAT network"): the scalar pieces of the bit-defined rule ----------
// Shared by k_train_rows / k_train_reduce_adam and the host flavour.  Every function that does float arithmetic for the rule opens
// with GBL_FP_STRICT, and so do the two kernels and the host flavour's own loops (train_row, train_sum, gbl_cpu_train_step): hipcc
// (and clang++ as a host compiler) must not contract a multiply and an add into an fma there -- the rule is single operations; g++
// takes the same from -ffp-contract=off (CPU_CXX_FLAGS).  HIPCC_FLAGS stay as they are.
#ifdef GBL_HOST_EMU
#ifndef __host__
#define __host__
#endif
#endif
#define GBL_FP_STRICT _Pragma("clang fp contract(off)")

constexpr int kTrainOutputs = 55;     // o_0 .. o_53: the action logits, o_54: the value
constexpr int kTrainDoStride = 56;    // the workspace's do rows (element 55 is padding, written as 0)
constexpr int kTrainRowStats = 4;     // the workspace's per-row record: lp, lv, the row's largest h, counted (1.0 / 0.0)
constexpr int kTrainChunk = 64;       // rows per chunk of the row sums
constexpr int64_t kTrainMaxBatch = 65536;

struct TrainHyper {  // gbl_train_hyper, as the kernels take it (by value)
    float lr, beta1, beta2, eps, weight_decay, value_reg, bias1, bias2;
};

inline bool train_hidden_ok(int h) { return h == 64 || h == 128 || h == 192 || h == 256; }
constexpr int train_param_count(int h) { return (kObs + 1 + kTrainOutputs) * h + kTrainOutputs; }
// floats of workspace: h [B][H], dh [B][H], do [B][56], the row records [B][4]
inline int64_t train_workspace_bytes(int64_t batch, int hidden)
{
    if (batch < 1 || batch > kTrainMaxBatch || !train_hidden_ok(hidden)) return 0;
    return 4 * batch * (2 * (int64_t)hidden + kTrainDoStride + kTrainRowStats);
}

inline const char *train_error(const void *obs, const void *visits, const void *z, int64_t batch, int hidden, const void *params,
                               const void *adam_m, const void *adam_v, const void *hyper, const void *stats_out, const void *workspace,
                               int64_t workspace_bytes)
{
    if (!train_hidden_ok(hidden)) return "hidden must be 64, 128, 192 or 256";
    if (batch < 1 || batch > kTrainMaxBatch) return "batch must be in [1, 65536]";
    if (!obs) return "obs must not be NULL";
    if (!visits) return "visits must not be NULL";
    if (!z) return "z must not be NULL";
    if (!params) return "params must not be NULL";
    if (!adam_m || !adam_v) return "adam_m / adam_v must not be NULL";
    if (!hyper) return "hyper must not be NULL";
    if (!stats_out) return "stats_out must not be NULL";
    if (!workspace) return "workspace must not be NULL";
    if (workspace_bytes < train_workspace_bytes(batch, hidden)) return "workspace_bytes is below gbl_train_workspace_bytes";
    return nullptr;
}

__host__ __device__ __forceinline__ float train_bits_float(uint32_t u) { return __builtin_bit_cast(float, u); }
__host__ __device__ __forceinline__ uint32_t train_float_bits(float f) { return __builtin_bit_cast(uint32_t, f); }

constexpr float kTrainLog2e = 0x1.715476p+0f, kTrainLn2Hi = 0x1.62e4p-1f, kTrainLn2Lo = 0x1.7f7d1cp-20f;

// EXP of the header: x <= 0 (a NaN or anything below -110 is taken as -110, whose result is 0)
__host__ __device__ __forceinline__ float train_exp(float x)
{
    GBL_FP_STRICT
    x = x >= -110.0f ? x : -110.0f;
    x = x <= 0.0f ? x : 0.0f;
    const float t = x * kTrainLog2e;
    const int32_t n = (int32_t)(t - 0.5f);
    const float fn = (float)n;
    const float r = (x - fn * kTrainLn2Hi) - fn * kTrainLn2Lo;
    float q = 0x1.a01a02p-13f;
    q = q * r; q = q + 0x1.6c16c2p-10f;
    q = q * r; q = q + 0x1.111112p-7f;
    q = q * r; q = q + 0x1.555556p-5f;
    q = q * r; q = q + 0x1.555556p-3f;
    q = q * r; q = q + 0x1p-1f;
    float y = r * r;
    y = y * q;
    y = y + r;
    y = y + 1.0f;
    const int32_t n1 = n >> 1, n2 = n - n1;
    y = y * train_bits_float((uint32_t)(n1 + 127) << 23);
    return y * train_bits_float((uint32_t)(n2 + 127) << 23);
}

// LOG of the header: s >= 1 and finite (anything else gives an unspecified float, never a fault)
__host__ __device__ __forceinline__ float train_log(float s)
{
    GBL_FP_STRICT
    const uint32_t u = train_float_bits(s);
    int32_t e = (int32_t)(u >> 23) - 127;
    const uint32_t mant = u & 0x7FFFFFu;
    const bool upper = mant > 0x3504F3u;
    e += upper ? 1 : 0;
    const float w = train_bits_float(mant | (upper ? 0x3F000000u : 0x3F800000u));
    const float f = w - 1.0f;
    const float q = f / (2.0f + f);
    const float y = q * q;
    float R = 0x1.c71c72p-3f;
    R = R * y; R = R + 0x1.24924ap-2f;
    R = R * y; R = R + 0x1.99999ap-2f;
    R = R * y; R = R + 0x1.555556p-1f;
    R = R * y;
    const float hf = (0.5f * f) * f;
    const float T = q * (hf + R);
    const float dk = (float)e;
    return (((T + dk * kTrainLn2Lo) - hf) + f) + dk * kTrainLn2Hi;
}

// the value column of a counted row: the loss term lv and do_54
__host__ __device__ __forceinline__ void train_value(float v, int z, float value_reg, float &lv, float &dv)
{
    GBL_FP_STRICT
    const float c = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
    const float u = c - (float)z;
    lv = u * u + value_reg * (v * v);
    dv = 2.0f * (v > -1.0f && v < 1.0f ? u : 0.0f) + 2.0f * (value_reg * v);
}

// one action of a counted row's candidate set: do_a and its term of the policy loss
__host__ __device__ __forceinline__ void train_policy(float e, float s, float d, float L, int visits, int S, float &da, float &term)
{
    GBL_FP_STRICT
    const float t = (float)visits / (float)S;
    da = e / s - t;
    term = t * (L - d);
}

// g of the header from a row sum, and Adam on one element
__host__ __device__ __forceinline__ float train_gradient(float G, float M, float theta, const TrainHyper &hy)
{
    GBL_FP_STRICT
    return G / M + hy.weight_decay * theta;
}

__host__ __device__ __forceinline__ void train_adam(float g, float &theta, float &m, float &v, const TrainHyper &hy)
{
    GBL_FP_STRICT
    m = hy.beta1 * m + (1.0f - hy.beta1) * g;
    v = hy.beta2 * v + (1.0f - hy.beta2) * (g * g);
    const float root = __builtin_sqrtf(v / hy.bias2);  // (correctly rounded on either side: hipcc's default for fp32 divide and sqrt)
    theta = theta - (hy.lr * (m / hy.bias1)) / (root + hy.eps);
}

// ---- gbl_train_step_weighted / gbl_replay_importance (include/gobblet_hip.h): the scalar pieces they add to the rule above -------------
constexpr float kTrainFltMax = 0x1.fffffep+127f;
constexpr int32_t kTrainPrioTop = 1 << 30;  // the most a loss can add to prio_floor
constexpr int64_t kImportanceMaxBatch = 65536;

// the effective weight ww of a row: a NaN, a negative, a zero and +inf all count 0
// (on the bits, which order as the positive floats do, so that a wavefront-uniform weight stays in the kernel's scalar registers:
// 0 < w <= FLT_MAX exactly where 0 < bits <= 0x7F7FFFFF as an int32 -- denormals included, -0 and every NaN excluded)
__host__ __device__ __forceinline__ uint32_t train_weight_bits(uint32_t u) { return (int32_t)u > 0 && (int32_t)u <= 0x7F7FFFFF ? u : 0u; }
__host__ __device__ __forceinline__ float train_weight(float w) { return train_bits_float(train_weight_bits(train_float_bits(w))); }

// prio_out of a counted row from its two unweighted loss terms
__host__ __device__ __forceinline__ int32_t train_priority(float lp, float lv, float scale, int32_t floor, int32_t cap)
{
    GBL_FP_STRICT
    float q = lp + lv;
    q = q * scale;
    const int32_t k = !(q > 0.0f) ? 0 : q >= 0x1p30f ? kTrainPrioTop : (int32_t)q;
    const int64_t p = (int64_t)floor + k;
    return (int32_t)(p < (int64_t)cap ? p : (int64_t)cap);
}

// what gbl_train_step_weighted checks after train_error (and, on the device, after gbl_train_step's alignment rules)
inline const char *train_weighted_error(const void *prio_out, float prio_scale, int32_t prio_floor, int32_t prio_cap)
{
    if (!prio_out) return nullptr;
    if (!(prio_scale >= 0.0f && prio_scale <= kTrainFltMax)) return "prio_scale must be finite and >= 0";
    if (prio_floor < 0 || prio_floor > prio_cap) return "prio_floor and prio_cap must satisfy 0 <= prio_floor <= prio_cap";
    return nullptr;
}

// the importance weight of a drawn row of priority p in a batch whose smallest positive priority is wmin (p > 0: wmin >= 1)
__host__ __device__ __forceinline__ float importance_weight(int32_t p, int32_t wmin, float beta)
{
    GBL_FP_STRICT
    if (p <= 0) return 0.0f;
    const float ratio = (float)p / (float)wmin;
    const float x = beta * train_log(ratio);
    return train_exp(-x);
}

inline const char *replay_importance_error(const void *prio, int64_t batch, float beta, const void *weights_out)
{
    if (batch < 1 || batch > kImportanceMaxBatch) return "batch must be in [1, 65536]";
    if (!(beta >= 0.0f && beta <= 1.0f)) return "beta must be in [0, 1]";
    if (!prio) return "prio must not be NULL";
    if (!weights_out) return "weights_out must not be NULL";
    return nullptr;
}

}  // namespace gbl
