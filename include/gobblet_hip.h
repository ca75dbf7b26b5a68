/*
 * gobblet_hip.h -- C-ABI of the MI355X (gfx950) batched Gobblet hot path.
 *
 * The reference (elliottower/gobblet-rl) is pure Python and has no FFI seam;
 * the seam this library sits behind is the `Board` object interface consumed
 * by gobblet_rl/game/gobblet.py, greedy_policy.py and manual_policy.py
 * (SURVEY.md section 8b).  Every entry point below is the lockstep, N-board
 * form of one reference function and cites it.  INTEGRATION.md shows the
 * ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - All pointers are DEVICE pointers owned by the caller (e.g. torch-ROCm
 *     tensors' data_ptr()).  The library keeps no state between calls, and the
 *     compute entry points allocate nothing and only enqueue on `stream`.  The
 *     exceptions are helpers, none of them on the step path:
 *     gbl_pinned_alloc / gbl_pinned_free and gbl_block_alloc / gbl_block_free
 *     allocate and free memory the CALLER then owns (the library keeps no
 *     reference), and gbl_placement_probe creates HIP events for its own
 *     duration and BLOCKS the host until its measurement has run.
 *   - Every buffer that holds per-board ROWS (state, mask, obs, flat, cov)
 *     must be 16-byte aligned at board 0 (hipMalloc / torch allocations are).
 *   - `stream` is a hipStream_t (NULL = default stream).  Calls only enqueue.
 *   - Return value: 0 = OK, negative = GBL_ERR_*; gbl_last_error() gives the
 *     thread-local message.  No C++ exception crosses the ABI.
 *   - Kernels never trap on bad data: an action outside [0,54) is an illegal
 *     action (handled per `illegal_mode`) and is flagged in the status byte of
 *     gbl_step_ex / gbl_collect_from_ex (GBL_STATUS_OUT_OF_RANGE).
 *
 * Threading and devices
 *   - The library is re-entrant and holds no global state: any number of host
 *     threads may call any entry points at the same time, each on buffers and
 *     a stream of its own.  The error text is per thread: gbl_last_error()
 *     returns what the CALLING thread's last failing call left, "" on a
 *     thread that has had none.
 *   - A call lands on the device that owns `stream` (NULL: the current
 *     device's default stream), and every launch and memset of a call --
 *     the multi-launch entry points included -- goes to that one stream, so
 *     any call can be captured into a hipGraph.  The CALLER makes that
 *     device current (hipSetDevice) before the call; the pointers must be
 *     that device's memory.  The Python classes do this themselves: an
 *     object launches on its own device whichever device is current, on the
 *     calling thread's current stream of that device.
 *   - One OBJECT of a caller -- a set of boards, a replay ring with its
 *     workspace, a network with its moments, a trainer's or a collector's
 *     staging buffers -- must not be driven from two threads at once: the
 *     calls are independent, the memory they are handed is not.
 *   (tests/test_host_threads.py, tests/test_gpu_devices_threads.py)
 *
 * Data layout in HBM (env-major, int8)
 *   state   int8 [n][27]      Board.squares per board: squares[9*level + pos]
 *                             (board.py:6-33); 0 empty, +piece player_1,
 *                             -piece player_2, piece in 1..6.
 *   to_move int8 [n]          index of agent_selection (0 = player_1)
 *   done    int8 [n]          terminations (both agents at once, gobblet.py:263)
 *   winner  int8 [n]          check_for_winner(): -1 / 0 / +1
 *   reward  int8 [n][2]       rewards of (player_1, player_2) for this step
 *   mask    int8 [n][54]      action_mask of the agent to move
 *   obs     int8 [n][3][3][13] observation of the agent to move
 *   actions int32[n]
 *   turn    int32[n]          raw_env.turn (plies since reset), optional
 * Contract on `state`: a cell of level k holds 0 or +-(2k+1) or +-(2k+2) --
 * what legal play from reset can produce.  For such states every function is
 * bit-identical to the reference.  Outside it nothing is promised (gbl_validate
 * flags such boards); in particular gbl_collect on small batches keeps the
 * boards as bit planes and REBUILDS the state rows from them on return, so a
 * cell that held a value its level cannot hold comes back as the contract's
 * reading of it (sign and parity kept), where larger batches leave it as found.
 */
#ifndef GOBBLET_HIP_H
#define GOBBLET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GBL_OK 0
#define GBL_ERR_ARG (-1)   /* null / negative / out-of-range argument */
#define GBL_ERR_ALIGN (-2) /* a row buffer is not 16-byte aligned */
#define GBL_ERR_HIP (-3)   /* a HIP runtime call failed; see gbl_last_error() */
/* Where an entry point's argument contract lives: its rules that both flavours have are one <name>_error() in
 * gobblet-rl_amd/csrc/gobblet_device.h, in the order they are reported; the device flavour's alignment rules follow in gobblet_hip.hip.
 * For gbl_reset ... gbl_greedy_act_at and the device-memory helpers tests/golden/env_arg_errors.json pins every rule, the order and
 * the early returns on both flavours (tests/test_abi_and_host.py replays it), as the other tests/golden/ *_arg_errors.json tables do
 * for the later families. */

#define GBL_CELLS 27
#define GBL_ACTIONS 54
#define GBL_OBS_BYTES 117

/* gbl_rollout tallies: int64[GBL_COUNTER_STRIPES][GBL_COUNTER_STRIDE]; words 0..3 of every
 * stripe hold {plies played, games finished, player_1 wins, player_2 wins}; a total is the
 * sum over stripes.  (Striped so that concurrently finishing wavefronts do not serialise on
 * one address; one stripe per 128-byte line.) */
#define GBL_COUNTER_STRIPES 64
#define GBL_COUNTER_STRIDE 16

/* illegal_mode */
#define GBL_ILLEGAL_NOOP 0      /* raw_env.step: silent no-op, the turn still passes (gobblet.py:244-246, board.py:125-126) */
#define GBL_ILLEGAL_TERMINATE 1 /* env(): TerminateIllegalWrapper(illegal_reward=-1) (gobblet.py:114, :50-51) */

/* Version / layout query: writes {abi_version, cells, actions, obs_bytes, tile_boards, row_alignment}.
 * abi_version 2 (round 6): + gbl_step_ex, gbl_collect_from_ex, GBL_STATUS_*; gbl_collect_variant reports GBL_COLLECT_TRIO as 4
 * (3, once GBL_COLLECT_SMALL, is retired).  Every entry point of version 1 keeps its signature and meaning. */
#define GBL_ABI_VERSION 2
int gbl_layout_info(int32_t out[6]);

/* Message of the last error on this thread ("" if none). */
const char *gbl_last_error(void);

/* raw_env.reset(), gobblet.py:275-290: new Board() (zeros, board.py:33),
 * agent_selection = player_1, terminations False.  winner may be NULL. */
int gbl_reset(int8_t *state, int8_t *to_move, int8_t *done, int8_t *winner, int64_t n, void *stream);

/* raw_env._legal_moves() + mask fill, gobblet.py:223-228,211-213
 * (54 x Board.is_legal, board.py:82-115) for agent to_move[b]. */
int gbl_legal_mask(const int8_t *state, const int8_t *to_move, int8_t *mask, int64_t n, void *stream);

/* Board.is_legal(action, agent_index), board.py:82-115, one action per board.
 * agent_index: device int8[n]; out: int8[n] (1 legal / 0 illegal or out of range). */
int gbl_is_legal(const int8_t *state, const int8_t *agent_index, const int32_t *actions, int8_t *out, int64_t n,
                 void *stream);

/* Board.play_turn(agent_index, action), board.py:118-132: in-place, silent no-op when illegal. */
int gbl_play_turn(int8_t *state, const int8_t *agent_index, const int32_t *actions, int64_t n, void *stream);

/* Board.check_for_winner(), board.py:183-194 (lines board.py:135-153; the last matching line decides). */
int gbl_winner(const int8_t *state, int8_t *winner, int64_t n, void *stream);

/* Board.get_flatboard(), board.py:159-177: flat int8[n][9], signed piece number of the top piece. */
int gbl_flatboard(const int8_t *state, int8_t *flat, int64_t n, void *stream);

/* Board.check_covered(), board.py:203-220: cov int8[n][27]. */
int gbl_covered(const int8_t *state, int8_t *cov, int64_t n, void *stream);

/* State-contract check for callers that assign `state` themselves (the reference lets callers
 * assign Board.squares: greedy_policy.py:71, manual_policy.py:60).  flags int8[n]: bit 0 = a cell
 * holds a value its level cannot hold; bit 1 = a piece number occurs twice, where the reference's
 * is_legal raises Exception("PIECE HAS BEEN USED TWICE") (board.py:94-95).  0 = board is valid. */
int gbl_validate(const int8_t *state, int8_t *flags, int64_t n, void *stream);

/* raw_env.observe(agent)["observation"], gobblet.py:179-208.
 * agent_sel = 0 / 1: observe every board as that agent; -1: as to_move[b]
 * (to_move may be NULL unless agent_sel == -1). */
int gbl_observe(const int8_t *state, const int8_t *to_move, int agent_sel, int8_t *obs, int64_t n, void *stream);

/* One lockstep raw_env.step(actions[b]) + observe(next mover) per board,
 * gobblet.py:231-271 + :179-215, fused.  In place on state / to_move / done.
 *   done[b] != 0 on entry: the board is frozen (reference: _was_dead_step,
 *     gobblet.py:232-236); its mask is written as zeros, obs as observed.
 *   auto_reset != 0: `done` on entry is ignored; a board that terminates on
 *     this step reports winner / reward / done = 1 and is reset in place
 *     (zeros, player_1 to move); mask / obs are those of the fresh board.
 *   turn (int32[n], in/out, may be NULL): raw_env.turn per board -- +1 whenever raw_env.step
 *     runs (also on an illegal no-op, gobblet.py:270), 0 after a reset (gobblet.py:289).
 *   winner_out / reward_out / mask_out / obs_out may each be NULL. */
int gbl_step(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *actions, int8_t *winner_out,
             int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int32_t *turn, int64_t n, int illegal_mode,
             int auto_reset, void *stream);
/* gbl_step for a collector whose policy lives outside the library (the loop of the reference's Tianshou / RLlib
 * trainers: policy(obs, mask) -> env.step -> buffer.add): the same ply, with mask_out / obs_out / winner_out /
 * reward_out pointing at slot t of trajectory arrays, and in the same launch copies of the ply's other scalars into
 * that slot (each may be NULL): actions_out int32[n] = the actions played, done_out int8[n] = done after the ply,
 * to_move_out int8[n] = the agent to move next. */
int gbl_step_into(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *actions, int8_t *winner_out,
                  int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int32_t *turn, int32_t *actions_out,
                  int8_t *done_out, int8_t *to_move_out, int64_t n, int illegal_mode, int auto_reset, void *stream);

/* gbl_step_into with two more optional outputs (each may be NULL; all NULL = gbl_step_into):
 *   status_out int8[n]: what became of actions[b] -- 0 = a legal move, played; GBL_STATUS_ILLEGAL = not a legal move of
 *     the mover (handled per illegal_mode: raw_env.step's silent no-op, gobblet.py:244-246 / board.py:125-126, or
 *     TerminateIllegalWrapper's -1, gobblet.py:114); GBL_STATUS_ILLEGAL | GBL_STATUS_OUT_OF_RANGE = outside [0, 54),
 *     where the reference's env() asserts (AssertOutOfBoundsWrapper, gobblet.py:110-117) -- the kernels never trap, a
 *     batched caller tells "illegal" from "garbage index" here.  A board that was frozen on entry consumes no action: 0.
 *   next_actions_out int32[n]: the NEXT mover's masked-uniform draw from the mask this very launch stores -- exactly
 *     gbl_sample_at(mask_out, next_actions_out, n, seed, env_base, ply, ply_dev) run behind the step (-1 where nobody
 *     is to move), without the sampler's launch and its 58 bytes per board of traffic: the random opponent's reply /
 *     an epsilon-greedy policy's exploration move of the reference's trainer loops (examples/example_basic.py:58-61,
 *     example_tianshou_DQN.py: MultiAgentPolicyManager([agent, RandomPolicy])).  May alias `actions`: a board's action
 *     is read before its next one is written, so one array can carry a masked-random game from launch to launch.
 *     mask_out may be NULL (the draw is taken from the same 54-bit set either way). */
#define GBL_STATUS_ILLEGAL 1
#define GBL_STATUS_OUT_OF_RANGE 2
int gbl_step_ex(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *actions, int8_t *winner_out,
                int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int32_t *turn, int32_t *actions_out,
                int8_t *done_out, int8_t *to_move_out, int8_t *status_out, int32_t *next_actions_out, uint64_t seed,
                uint64_t env_base, uint32_t ply, const uint32_t *ply_dev, int64_t n, int illegal_mode, int auto_reset,
                void *stream);

/* Host memory that the kernels read and write directly (pinned and mapped into the device's address space), for
 * callers that want a result on the host without a separate copy -- the single-environment facade keeps its
 * board, action and 432-byte record there, so a ply crosses PCIe inside its one launch.  *host_ptr is the CPU's
 * view, *dev_ptr the pointer to hand to the gbl_* entry points (same memory).  The caller owns the block and
 * frees it with gbl_pinned_free(host_ptr); the library keeps no reference. */
int gbl_pinned_alloc(int64_t bytes, void **host_ptr, void **dev_ptr);
int gbl_pinned_free(void *host_ptr);

/* Everything the reference derives from a position, for n boards, in ONE launch (the single-environment
 * facade gobblet_v1.env() asks all of it once per ply): optionally Board.play_turn(agent_index[b], actions[b])
 * first (board.py:118-132; illegal or out-of-range: silent no-op; `state` is updated in place), then one
 * GBL_REC_BYTES-byte record per board of the resulting position:
 *   +GBL_REC_SQUARES int8[27]  Board.squares                     board.py:33
 *   +GBL_REC_WINNER  int8      check_for_winner()                board.py:183-194
 *   +GBL_REC_FLAT    int8[9]   get_flatboard()                   board.py:159-177
 *   +GBL_REC_COVERED int8[27]  check_covered()                   board.py:203-220
 *   +GBL_REC_MASK0 / +GBL_REC_MASK1  int8[54]  is_legal(a, agent 0 / 1), a = 0..53   board.py:82-115
 *   +GBL_REC_OBS0  / +GBL_REC_OBS1   int8[117] raw_env.observe planes of agent 0 / 1   gobblet.py:179-208
 * (every field 4-byte aligned, padding bytes zero).  actions == NULL: no move (agent_index is then unused and
 * may be NULL).  record_out: int8[n][GBL_REC_BYTES], 16-byte aligned. */
#define GBL_REC_BYTES 432
#define GBL_REC_SQUARES 0
#define GBL_REC_WINNER 28
#define GBL_REC_FLAT 32
#define GBL_REC_COVERED 44
#define GBL_REC_MASK0 72
#define GBL_REC_MASK1 128
#define GBL_REC_OBS0 184
#define GBL_REC_OBS1 304
int gbl_board_eval(int8_t *state, const int8_t *agent_index, const int32_t *actions, int8_t *record_out, int64_t n,
                   void *stream);

/* Masked-uniform action sampling -- the rule behind "masked-random actions"
 * (examples/example_basic.py:58-61, random_admissible_policy_rllib.py:23-30:
 * uniform over legal actions) -- with a counter-based RNG so CPU and GPU draw
 * the same action: r = word (ply & 3) of Philox4x32-10(ctr = (env_lo, env_hi,
 * ply >> 2, stream), key = (seed_lo, seed_hi)) -- one generator block serves four
 * consecutive plies of a board; k = (r * nlegal) >> 32; the k-th legal action
 * in ascending order (-1 if the mask is empty).  env id = env_base + b.
 * Counter word 3 separates the consumers of one (seed, board) pair: stream 0 here
 * and in gbl_rollout, stream 1 for the fallback draw of gbl_greedy_act, stream 2
 * for the playouts of gbl_playout_values. */
int gbl_sample(const int8_t *mask, int32_t *actions, int64_t n, uint64_t seed, uint64_t env_base, uint32_t ply,
               void *stream);

/* Fused masked-random rollout: `plies` lockstep plies in ONE
 * launch; per ply and board: legal mask -> gbl_sample rule with ply index
 * ply0 + t -> gbl_step with auto-reset.  The board stays in registers between
 * plies; state / to_move / done and the optional outputs (action, winner,
 * reward, mask, obs of the agent to move) are stored after the LAST ply.
 * plies = 1 is "sample + step" fused into one launch: every ply's outputs
 * are then materialised in HBM for a consumer, as with gbl_sample + gbl_step.
 * counters: device int64[GBL_COUNTER_STRIPES][GBL_COUNTER_STRIDE], 128-byte
 * aligned, atomically incremented (see above; may be NULL -- the atomics cost
 * a few microseconds per launch at 2^20 boards).  turn: as in gbl_step (may be
 * NULL).  actions_out / winner_out / reward_out / mask_out / obs_out may be NULL. */
int gbl_rollout(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_out, int8_t *winner_out,
                int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int64_t n, uint64_t seed, uint64_t env_base,
                uint32_t ply0, uint32_t plies, int illegal_mode, int64_t *counters, int32_t *turn, void *stream);

/* GreedyGobbletPolicy.compute_action board decode, greedy_policy.py:43-71:
 * obs int8[n][3][3][13] -> state int8[n][27], to_move int8[n] (channel 12). */
int gbl_decode_obs(const int8_t *obs, int8_t *state, int8_t *to_move, int64_t n, void *stream);

/* GreedyGobbletPolicy.compute_action, greedy_policy.py:38-221, depth 1, 2 or
 * 3, for the agent to move on each board.  depth 3 returns the depth-2
 * decision: the only assignment in the reference's depth-3 block (:160-208)
 * is `chosen_action = action` (:197), which :157 has just made, and
 * actions_depth3 is local, so that block cannot change the result (pinned on
 * the reference itself by tests/golden/greedy_depth3.npz).
 *   mask     : legal mask handed to the policy (NULL = derive from state)
 *   hist     : int8[n][2][3] last three actions per agent, -1 = none (NULL = empty)
 *   action_out   int32[n] : chosen action; -1 where the reference falls back
 *                           to np.random.choice(actions_depth1) (:211-217)
 *   cand_mask_out int8[n][54] : membership of actions_depth1 at :211 (may be NULL)
 *   fallback_out  int8[n]     : 1 where the fallback fires (may be NULL) */
int gbl_greedy(const int8_t *state, const int8_t *to_move, const int8_t *mask, const int8_t *hist, int depth,
               int32_t *action_out, int8_t *cand_mask_out, int8_t *fallback_out, int64_t n, void *stream);

/* One whole policy step of GreedyGobbletPolicy.compute_action, greedy_policy.py:38-221, in one launch:
 * gbl_greedy, then where it reports the fallback (:211-217) the gbl_sample rule over the candidate set
 * with (seed, env_base + b, call) on generator stream 1 in place of numpy's global RNG (so a random opponent
 * sampling with the same seed never consumes the same word), then the history append of :219
 * (hist[b][agent to move] shifts left by one and takes the returned action).
 *   hist      : int8[n][2][3], read AND updated (required)
 *   action_out  int32[n] : the action the policy returns (-1 only if the candidate set is empty)
 *   chosen_out  int32[n] : gbl_greedy's action_out (chosen, or -1 where the fallback fired; may be NULL)
 *   cand_mask_out / fallback_out : as gbl_greedy (may be NULL) */
int gbl_greedy_act(const int8_t *state, const int8_t *to_move, const int8_t *mask, int8_t *hist, int depth,
                   uint64_t seed, uint64_t env_base, uint32_t call, int32_t *action_out, int32_t *chosen_out,
                   int8_t *cand_mask_out, int8_t *fallback_out, int64_t n, void *stream);

/* Graph-replay forms of the three entry points that draw random numbers.  seed / env_base / ply travel by value,
 * so a captured hipGraph would replay the same draws; here the index is  ply + *ply_dev  (call + *call_dev) with
 * the base in device memory, and gbl_counter_add -- one more node at the end of the captured sequence -- moves
 * it on, so every replay draws afresh.  A NULL pointer makes them the by-value forms. */
int gbl_sample_at(const int8_t *mask, int32_t *actions, int64_t n, uint64_t seed, uint64_t env_base, uint32_t ply,
                  const uint32_t *ply_dev, void *stream);
int gbl_rollout_at(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_out, int8_t *winner_out,
                   int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int64_t n, uint64_t seed, uint64_t env_base,
                   uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int illegal_mode, int64_t *counters,
                   int32_t *turn, void *stream);
int gbl_greedy_act_at(const int8_t *state, const int8_t *to_move, const int8_t *mask, int8_t *hist, int depth,
                      uint64_t seed, uint64_t env_base, uint32_t call, const uint32_t *call_dev, int32_t *action_out,
                      int32_t *chosen_out, int8_t *cand_mask_out, int8_t *fallback_out, int64_t n, void *stream);

/* Flat Monte-Carlo playout values (no counterpart in the reference: a stronger, tunable opponent than the greedy policy, and
 * the leaf evaluator / value target of a tree search).  For every candidate action a of board b -- mask[b] & legal mask of
 * the agent to move (mask NULL: the legal mask) -- and every k < playouts:
 *   1. the mover plays a; a non-zero check_for_winner() decides the playout (a win, or a loss by uncovering an opponent's line);
 *   2. else, for t = 1 .. max_plies, the side to move plays the gbl_sample rule over its legal mask with the generator word of
 *      (seed, pid, ply index (call << 8) | t, stream 2), pid = ((env_base + b) * 54 + a) * 65536 + k, until the first non-zero
 *      winner; max_plies plies without one, or no legal move, leave the playout unfinished.
 * Outputs (each may be NULL; non-candidate entries are 0):
 *   wins_out   int32[n][54] : playouts of a won by the mover       losses_out int32[n][54] : ... lost by the mover
 *   action_out int32[n]     : the candidate with the largest wins - losses, the lowest index on ties; -1 without a candidate
 *   plies_out  int32[n]     : plies played over all of b's playouts, the root moves included
 * pid does not depend on `playouts`, so the counts are non-decreasing in it, and a shard (env_base) of a batch gets its
 * boards' results.  1 <= playouts <= 4096, 0 <= max_plies <= 255, call < 2^24, env_base + n <= 2^42; states must be
 * contract states (gbl_validate).  state / to_move / mask are read a byte at a time and need NO alignment here (the
 * 16-byte rule above is for the entry points that move whole rows); the outputs must be 4-byte aligned (GBL_ERR_ALIGN).
 * to_move and mask count as set wherever they are non-zero.  Allocates nothing. */
int gbl_playout_values(const int8_t *state, const int8_t *to_move, const int8_t *mask, int playouts, int max_plies,
                       uint64_t seed, uint64_t env_base, uint32_t call, int32_t *wins_out, int32_t *losses_out,
                       int32_t *action_out, int32_t *plies_out, int64_t n, void *stream);

/* UCT tree search (no counterpart in the reference): leaf-parallel, one independent tree per board, `iterations` leaves of
 * `playouts` masked-random playouts each.  Deterministic and integer-only (every operand below 2^64, every division an unsigned
 * integer division of non-negative operands), so that the kernel, the host flavour and a restatement of this text agree bit for bit.
 * Per board g = env_base + b with mover m = to_move[b], P = playouts:
 *   Nodes.  Node 0 is the root (the given position, m to move); every other node is the position after its parent's side played
 *     one action.  A node keeps n_v (iterations that went through it) and W_v, L_v (playout outcomes counted for the side that
 *     moved INTO the node).  A node other than the root is terminal if check_for_winner() is non-zero after the move into it, or
 *     if its side to move has no legal action.  The root's candidates are mask[b] & its legal mask (mask NULL: the legal mask);
 *     every other node's candidates are its legal mask.  A root without a candidate: nothing is played, action_out = -1,
 *     nodes_out = 1, everything else 0.
 *   Iteration i = 0 .. iterations - 1:
 *     1. Select.  Start at the root.  While the node is not terminal and every candidate has a child, go to the child c with the
 *        largest key, the lowest action on ties:
 *          key(c) = (((W_c - L_c + n_c P) << 15) / (n_c P)) + ((explore * isqrt((bitlen(n_p) << 20) / n_c)) >> 3)
 *        p = the node being left, bitlen(x) = 32 - clz(x), isqrt = the exact integer square root.  The first term is the child's
 *        mean outcome for the side choosing, 0 .. 65536; the second is UCB1's exploration term with the logarithm replaced by the
 *        bit length; explore is in units of 1/256 of a full win.
 *     2. Expand.  If the node reached is not terminal: one of its candidates without a child by the gbl_sample rule
 *        (k = (r * count) >> 32, the k-th such action ascending), r = the generator word of (seed, pid(g, i, 0), ply index
 *        (call << 8) | 0, stream 3), pid(g, i, j) = (g * 1024 + i) * 256 + j; the child is created.
 *     3. Evaluate the leaf (the new child, or the terminal node selection stopped at).  Decided by check_for_winner(): all P
 *        outcomes are that result, nothing is played.  Its side has no move: all P outcomes are unfinished.  Otherwise playout
 *        j = 0 .. P - 1 starts from the leaf's position and plays, for t = 1 .. max_plies, the gbl_sample rule over the legal mask
 *        of the side to move with the generator word of (seed, pid(g, i, j), (call << 8) | t, stream 3), until the first
 *        non-zero winner; max_plies plies without one, or no legal move, leave it unfinished (neither a win nor a loss).
 *     4. Back up.  From the leaf to the root: n_v += 1, W_v += wins, L_v += losses, wins and losses swapping at every level; the
 *        root only counts n.
 * Outputs (each may be NULL), for the root's child c of action a, from the root mover's side; 0 for every other action:
 *   visits_out int32[n][54] = n_c      wins_out int32[n][54] = W_c      losses_out int32[n][54] = L_c
 *   action_out int32[n] : the root's child with the largest n_c, then the larger W_c - L_c, then the lowest action; -1 without one
 *   nodes_out  int32[n] : nodes created, the root included          plies_out int32[n] : masked-random plies played in all playouts
 * pid does not depend on `iterations`: a search is the beginning of every longer one, so nodes_out and the sum of visits_out do
 * not decrease with it, and a shard (env_base) of a batch gets its boards' results.  1 <= iterations <= 1024, 1 <= playouts <= 256,
 * 0 <= max_plies <= 255, 0 <= explore <= 1024, call < 2^24, env_base + n <= 2^42; states must be contract states (gbl_validate).
 * state / to_move / mask are read a byte at a time and need NO alignment here (as gbl_playout_values); the outputs must be 4-byte
 * aligned (GBL_ERR_ALIGN).  to_move and mask count as set wherever they are non-zero.
 * Allocates nothing; the tree lives in 16 (iterations + 1) bytes of LDS per workgroup. */
int gbl_tree_search(const int8_t *state, const int8_t *to_move, const int8_t *mask, int iterations, int playouts, int max_plies,
                    int explore, uint64_t seed, uint64_t env_base, uint32_t call, int32_t *visits_out, int32_t *wins_out,
                    int32_t *losses_out, int32_t *action_out, int32_t *nodes_out, int32_t *plies_out, int64_t n, void *stream);

/* A small integer network that evaluates a position (no counterpart in the reference): 117 observation bytes -> H hidden units ->
 * 54 action logits and a value.  The struct lives on the HOST; its four pointers are DEVICE pointers (host pointers in the host
 * flavour), each 16-byte aligned (GBL_ERR_ALIGN), and the arrays are only read.
 *   hidden  H, one of 64, 128, 192, 256
 *   w1      int8  [117][H]       row f = the weights of observation byte f
 *   b1      int32 [H]            |b1| <= 2^20
 *   w2      int8  [H / 4][56][4] element [j / 4][k][j % 4] = the weight of hidden unit j for output k; outputs 0..53 are the action
 *                                logits, 54 is the value, 55 is padding: o_55 follows the same rule and nothing reads it
 *   b2      int32 [56]           |b2| <= 2^24
 *   shift1, shift_p, shift_v     each in 0 .. 24
 * The rule, for a position p with side s to move.  Integer-only: every shift is arithmetic (floor), every division an unsigned
 * integer division, every operand stays inside int32, so that the kernels, the host flavour and a restatement of this text agree
 * bit for bit.
 *   x     = the 117 observation bytes of p as s observes it (gbl_observe with agent_sel = s); they are 0 or 1, at most 21 are 1
 *   h_j   = clamp((b1_j + sum over f with x_f = 1 of w1[f][j]) >> shift1, 0, 127)                    j = 0 .. H - 1
 *   o_k   = b2_k + sum over j of h_j * w2(j, k)                                                      k = 0 .. 55
 *   value   q = clamp(o_54 >> shift_v, -128, 128), in 1/128 of a win for s
 *   priors over a candidate set C of actions, C not empty:
 *     l_a  = o_a >> shift_p                     (in 1/16 of an octave)
 *     d_a  = min(max over C of l - l_a, 255)
 *     e_a  = T[d_a & 15] >> (d_a >> 4),  T[k] = floor(65536 * 2^(-k / 16) + 0.5) =
 *            65536 62757 60097 57549 55109 52773 50535 48393 46341 44376 42495 40693 38968 37316 35734 34219
 *     pi_a = 1 + (e_a * 254) / (sum over C of e)    for a in C, a uint8 in 1 .. 255;  pi_a = 0 outside C */
typedef struct {
    const int8_t *w1;
    const int32_t *b1;
    const int8_t *w2;
    const int32_t *b2;
    int32_t hidden, shift1, shift_p, shift_v;
} gbl_evaluator;

/* The network alone, one evaluation per board from the side to move: C = mask[b] & the mover's legal mask (mask NULL: the legal
 * mask).  Outputs:
 *   priors_out uint8 [n][54] : pi over C; all zeros where C is empty        value_out int32[n] : q (also where C is empty)
 *   logits_out int32 [n][56] : o_0 .. o_55 (may be NULL)
 * state / to_move / mask are read a byte at a time and need NO alignment here (as gbl_tree_search); to_move and mask count as set
 * wherever they are non-zero; value_out / logits_out must be 4-byte aligned (GBL_ERR_ALIGN).  Allocates nothing. */
int gbl_evaluate(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, uint8_t *priors_out,
                 int32_t *value_out, int32_t *logits_out, int64_t n, void *stream);

/* Evaluator-guided tree search: gbl_tree_search with the network above in place of the playouts, and with its priors steering the
 * selection.  Deterministic and integer-only; it draws NOTHING -- there is no seed, no env_base and no call, two calls on the same
 * boards give the same result, and a board's result does not depend on the batch it is in.  One launch is one decision: nothing
 * persists between launches.  Per board with mover m = to_move[b], P = 128 throughout:
 *   Nodes.  Nodes, what makes a node terminal, W / L / n and the root's candidates are those of gbl_tree_search.  Every node that is
 *     not terminal also keeps the prior row pi over its own candidates, from the network's evaluation of the node's position (from
 *     its side to move) at the moment the node is created; the root is created before iteration 0, and its q is root_value_out.
 *     A root without a candidate: nothing is searched, action_out = -1, nodes_out = 1, the root's q is still written, everything
 *     else is 0.
 *   Iteration i = 0 .. iterations - 1:
 *     1. Select.  Start at the root.  At a node v that is not terminal every candidate a of v gets
 *          key(a) = mean + ((explore * pi_a * isqrt(n_v << 8)) >> 5) / (1 + n_c)
 *        where, if a has a child c, mean = ((W_c - L_c + n_c P) << 15) / (n_c P) (gbl_tree_search's first term), and otherwise
 *        mean = 32768 and n_c = 0.  Take the largest key, the lowest action on ties.  If that action has a child, go there and
 *        repeat; if not, that action is the expansion.  A terminal node stops the selection and is evaluated itself.
 *     2. Expand and evaluate.  The child is created.  Decided by check_for_winner() after the move: wins or losses = P, as in
 *        gbl_tree_search.  Its side has no move: 0 and 0.  Otherwise the network evaluates the child's position from its side to
 *        move, the child keeps that prior row (C = its legal mask), and for the side that moved INTO the child
 *        wins = max(-q, 0), losses = max(q, 0).  A terminal node reached again counts its P or 0 / 0 again.
 *     3. Back up.  As gbl_tree_search: n_v += 1, W_v += wins, L_v += losses from the leaf to the root, wins and losses swapping at
 *        every level; the root only counts n.
 * Outputs (each may be NULL): visits_out / wins_out / losses_out int32[n][54], action_out int32[n] (most visits, then the larger
 * W - L, then the lowest action; -1 without a candidate) and nodes_out int32[n] as gbl_tree_search; root_value_out int32[n] = the
 * root's q; root_priors_out uint8[n][54] = the root's prior row.
 * 1 <= iterations <= 512, 0 <= explore <= 1024; the evaluator as above; states must be contract states (gbl_validate).
 * state / to_move / mask are read a byte at a time and need NO alignment here; to_move and mask count as set wherever they are
 * non-zero; the int32 outputs must be 4-byte aligned (GBL_ERR_ALIGN).
 * Allocates nothing; the tree lives in 72 (iterations + 1) bytes of LDS per workgroup (16-byte nodes and 56-byte prior rows). */
int gbl_tree_search_eval(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                         int explore, int32_t *visits_out, int32_t *wins_out, int32_t *losses_out, int32_t *action_out,
                         int32_t *nodes_out, int32_t *root_value_out, uint8_t *root_priors_out, int64_t n, void *stream);

/* Root noise: gbl_tree_search_eval with a random row mixed into the ROOT's prior row, once per search (the exploration of a self-play
 * search).  Integer-only, drawn inside the launch, and keyed by (seed, board id, call) alone: a board's result does not depend on the
 * batch or the shard it is in.  Parameters: the weight w = `noise` in 0 .. 256, seed, the board id g = env_base + b and q = call.
 * C is the root's candidate set and pi the root's prior row, exactly as gbl_tree_search_eval computes them.
 *   w == 0   nothing is drawn and the search is gbl_tree_search_eval, bit for bit.
 *   w > 0    Draw.  For every a in C, r_a = the generator word of (seed, g, ply index 64 q + a, stream 6): gbl_sample's generator,
 *              the Philox block with counter (g_lo, g_hi, (64 q + a) >> 2, 6), word a & 3 -- one block serves four actions.  Stream 6
 *              is the noise's own; streams 0 .. 5 belong to the other consumers of a (seed, board) pair.
 *            Noise row.  nu = the prior rule of gbl_evaluator over C with l_a = -(r_a >> 24):
 *              d_a = (r_a >> 24) - min over C of (r >> 24),  e_a = T[d_a & 15] >> (d_a >> 4),  nu_a = 1 + (e_a * 254) / (sum over C of e),
 *              and nu_a = 0 outside C.  The e_a are log-uniform over 16 octaves.
 *            Mix.  pi'_a = (pi_a * (256 - w) + nu_a * w + 128) >> 8 for a in C, 0 outside; it stays in 1 .. 255, and w = 256 gives nu.
 *            The root node keeps pi' as its prior row, so that the selection at the root uses pi'.  Every other node keeps its
 *            network row.  Everything else is gbl_tree_search_eval's text unchanged: the iterations, the keys, the back-up,
 *            action_out.  The root's q is not touched.  A root without a candidate draws nothing.
 * Outputs: those of gbl_tree_search_eval -- root_priors_out stays the network's row pi -- and root_mixed_out uint8[n][54] (may be
 * NULL) = pi', which equals pi where noise == 0.
 * `call` travels by value: a replayed graph repeats its noise, as it repeats gbl_training_batch's draws.
 * noise outside 0 .. 256, call >= 2^24 (the ply index 64 q + a fits 32 bits) and env_base + n > 2^42 are GBL_ERR_ARG; every other
 * limit, the alignment rules and the LDS as gbl_tree_search_eval.  Allocates nothing. */
int gbl_tree_search_eval_noise(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                               int explore, int noise, uint64_t seed, uint64_t env_base, uint32_t call, int32_t *visits_out,
                               int32_t *wins_out, int32_t *losses_out, int32_t *action_out, int32_t *nodes_out, int32_t *root_value_out,
                               uint8_t *root_priors_out, uint8_t *root_mixed_out, int64_t n, void *stream);

/* Gumbel root search (no counterpart in the reference): gbl_tree_search_eval with the ROOT's selection, decision and policy target
 * replaced by the root rule of "Policy improvement by planning with Gumbel" (Danihelka, Guez, Schrittwieser, Silver, ICLR 2022) --
 * Gumbel noise once per root, the top-m actions by g + logit, the budget spent on them by sequential halving, and the completed-Q
 * improved policy as a dense target -- in integers, so that the kernel, the host flavour and a restatement of this text agree byte
 * for byte.  It is made for small budgets: 8 .. 16 iterations over up to 54 candidates.
 * Parameters: gbl_tree_search_eval's, plus `considered` in 1 .. 54, `gumbel_noise` in {0, 1}, `visit_offset` in 0 .. 255, `scale` in
 * 0 .. 64, and seed, the board id g = env_base + b and q = call as in gbl_tree_search_eval_noise.  C is the root's candidate set, o
 * the root evaluation's outputs and q_root its value, exactly as gbl_tree_search_eval computes them.  Everything below is for a in C.
 *   Gumbel row.  gumbel_noise == 0: g_a = 0 and nothing is drawn.  gumbel_noise == 1: g_a = GT[r_a >> 24], r_a = the generator word
 *     of (seed, g, ply index 64 q + a, stream 10) -- gbl_sample's generator, the Philox block with counter (g_lo, g_hi, (64 q + a) >> 2,
 *     10), word a & 3; stream 10 is the rule's own.  GT[k] = round(-ln(-ln((k + 1/2) / 256)) * 16 / ln 2), k = 0 .. 255: a standard Gumbel
 *     variate in the logits' unit of 1/16 of an octave (no entry lies within 0.003 of a rounding tie):
 *     -42 -38 -35 -34 -32 -31 -30 -29 -28 -28 -27 -26 -26 -25 -24 -24 -23 -23 -22 -22 -21 -21 -21 -20 -20 -19 -19 -19 -18 -18 -17 -17
 *     -17 -16 -16 -16 -15 -15 -15 -14 -14 -14 -14 -13 -13 -13 -12 -12 -12 -11 -11 -11 -11 -10 -10 -10 -10 -9 -9 -9 -8 -8 -8 -8
 *     -7 -7 -7 -7 -6 -6 -6 -6 -5 -5 -5 -5 -4 -4 -4 -4 -3 -3 -3 -3 -2 -2 -2 -2 -1 -1 -1 -1 0 0 0 0
 *     1 1 1 1 2 2 2 2 3 3 3 3 4 4 4 4 5 5 5 5 6 6 6 6 7 7 7 7 8 8 8 8
 *     9 9 9 9 10 10 10 10 11 11 11 12 12 12 12 13 13 13 13 14 14 14 15 15 15 15 16 16 16 17 17 17
 *     18 18 18 19 19 19 19 20 20 20 21 21 21 22 22 22 23 23 24 24 24 25 25 25 26 26 27 27 27 28 28 29
 *     29 29 30 30 31 31 32 32 33 33 33 34 34 35 35 36 37 37 38 38 39 39 40 41 41 42 43 43 44 45 45 46
 *     47 48 48 49 50 51 52 53 54 55 56 57 59 60 61 63 64 66 67 69 71 73 76 78 81 84 88 93 99 107 119 144
 *   Root logits.  l_a = o_a >> shift_p;  L_a = -min(max over C of l - l_a, 255) -- the prior rule's own cap.
 *   Completed value.  mean_a = ((W_c - L_c + n_c P) << 15) / (n_c P) of the root's child c of a (the selection key's first term, 0 ..
 *     65536, for the root's mover) if a has one, else mean_a = 32768 + 256 q_root.  maxN = the largest n among the root's children
 *     (0 without one).  sigma_a = ((visit_offset + maxN) * scale * mean_a) >> 16, inside uint32 (767 * 64 * 65536 < 2^32).
 *   Considered set.  m = min(considered, |C|); A = the m actions of C with the largest g_a + L_a, ties to the lower action;
 *     P = max(1, ceil(log2 m)); the visit target starts at T = max(1, iterations div (P m)).
 *   Iteration i = 0 .. iterations - 1.  Before its selection: if |A| > 2 and every action of A has a root child with n >= T, HALVE --
 *     keep the max(2, ceil(|A| / 2)) actions of A with the largest g_a + L_a + sigma_a (sigma evaluated now), ties to the lower
 *     action, then T += max(1, iterations div (P |A|)) with the new |A|.  At most one halving per iteration; none once |A| <= 2.
 *     Select: at the ROOT take the action of A with the fewest visits (0 without a child), ties to the larger g_a + L_a, then to the
 *     lower action.  Everywhere below the root, and for expansion, evaluation and back-up, the text of gbl_tree_search_eval holds
 *     unchanged.  The search stops after `iterations`, wherever the schedule stands.
 *   Decision.  Among A: the most visits, then the largest g_a + L_a + sigma_a at the end, then the lowest action.
 *   Target row.  t_a = L_a + sigma_a (no g; sigma at the end, an unvisited action through the root's value);
 *     target_a = 1 + (e_a * 254) / (sum over C of e), e_a = T[d & 15] >> (d >> 4) with d = min(max over C of t - t_a, 255): the prior
 *     rule over t, a byte in 1 .. 255; 0 outside C.
 *   A root without a candidate: nothing is drawn or searched, action_out = -1, the target and the Gumbel row are zeros, the rest as
 *     gbl_tree_search_eval.
 * Outputs (each may be NULL): those of gbl_tree_search_eval -- visits_out / wins_out / losses_out are the raw counts of the root's
 * children, action_out the decision above -- and target_out uint8[n][54], gumbel_out int16[n][54] = g_a (0 outside C; 2-byte aligned).
 * The rule keeps two registers per lane and A as a mask: the LDS is gbl_tree_search_eval's.
 * Errors, in this order: n < 0, call >= 2^24, env_base + n > 2^42, the evaluator's fields, iterations, explore (all as
 * gbl_tree_search_eval_noise), then considered, gumbel_noise, visit_offset, scale out of range (GBL_ERR_ARG); with n == 0 the call
 * returns here; then the pointers and alignments of gbl_tree_search_eval.  Allocates nothing. */
int gbl_tree_search_gumbel(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                           int explore, int considered, int gumbel_noise, int visit_offset, int scale, uint64_t seed, uint64_t env_base,
                           uint32_t call, int32_t *visits_out, int32_t *wins_out, int32_t *losses_out, int32_t *action_out,
                           int32_t *nodes_out, int32_t *root_value_out, uint8_t *root_priors_out, uint8_t *target_out, int16_t *gumbel_out,
                           int64_t n, void *stream);

/* Exact bounded-depth solver (no counterpart in the reference): the full-width game tree of every board to `depth` plies, the proven
 * result of every root action.  Integer-only and draws nothing: the kernel, the host flavour and a restatement of this text agree
 * byte for byte.
 *   Result of an action.  s = the side to move in a position, r >= 1 the plies left.  For a legal action a: play a, read
 *     w = check_for_winner() (with the reference's last-line-decides rule where a move uncovers a line of the opponent).  Then
 *       c(a) = +1  if w is s;          c(a) = -1  if w is the other side (a move that loses at once);
 *       c(a) =  0  if w == 0 and r == 1;
 *       otherwise, with u = V(position after a, other side, r - 1):  c(a) = 0 if u == 0, else -sign(u) * (|u| + 1).
 *   Value of a position.  V(position, s, r) = 0 if s has no legal action; otherwise the c(a) of largest rank, where
 *       rank(c) = 64 - c for c > 0,    rank(0) = 0,    rank(c) = -64 - c for c < 0:
 *     the shortest forced win, then the unproven, then the longest forced loss.  +k reads "the mover wins at ply k against every
 *     defence", -k "the mover has lost by ply k whatever they do", 0 "nothing is proven within r plies".
 * The root's candidates are mask[b] & the legal mask of to_move[b] (mask NULL: the legal mask), as in gbl_playout_values; below the
 * root the legal mask is used.  Outputs (each may be NULL):
 *   outcome_out int8[n][54] : c(a) with r = depth for every candidate a, GBL_SOLVE_NONE for every other action
 *   value_out   int8[n]     : the root's V; 0 without a candidate
 *   action_out  int32[n]    : the candidate of largest rank, the lowest index on ties; -1 without a candidate
 * An implementation may prune (a win in one ply ends a node; window cuts) only where every output byte stays that of the
 * full-width definition above: the contract is the definition, not the traversal.
 * 1 <= depth <= GBL_SOLVE_MAX_DEPTH; states must be contract states (gbl_validate).  state / to_move / mask are read a byte at a
 * time and need NO alignment; action_out must be 4-byte aligned (GBL_ERR_ALIGN); to_move and mask count as set wherever they are
 * non-zero.  n == 0 returns GBL_OK; n < 0 and null inputs GBL_ERR_ARG.  Allocates nothing. */
#define GBL_SOLVE_MAX_DEPTH 6
#define GBL_SOLVE_NONE (-128)
int gbl_solve(const int8_t *state, const int8_t *to_move, const int8_t *mask, int depth, int8_t *outcome_out, int8_t *value_out,
              int32_t *action_out, int64_t n, void *stream);

/* Trajectory collection (K plies per launch with EVERY ply materialised).  `plies` masked-random
 * plies with auto-reset in ONE launch; ply t (t = 0 .. plies-1) of board b leaves in element
 *     cell(t, b) = t * ply_stride + (b / 64) * tile_stride + b % 64
 * of the trajectory arrays exactly what gbl_rollout(plies = 1) with ply index ply0 + t leaves in element b of
 * its output arrays:
 *   actions_traj int32[cells]      the action played at ply t
 *   winner_traj  int8 [cells]      check_for_winner() after it        reward_traj int8[cells][2]
 *   done_traj    int8 [cells]      1 where the episode ended on ply t (the board was then reset)
 *   to_move_traj int8 [cells]      the agent to move next -- the one mask / obs of the element belong to
 *   mask_traj    int8 [cells][54]  obs_traj int8[cells][117]
 * (any of them may be NULL).  The two strides, in boards and multiples of 16, choose the layout:
 *   time-major  [plies][slot_boards]:  ply_stride = slot_boards >= n rounded up to 64, tile_stride = 64
 *                                      (element (t, b) at t * slot_boards + b: one array slice per ply);
 *   tile-major  [tiles][plies][64]:    ply_stride = 64, tile_stride = 64 * plies
 *                                      (each tile of 64 boards keeps its whole trajectory contiguous: every
 *                                      wavefront writes ONE sequential region per array).
 * state / to_move / done / turn / counters are read at entry and hold the position after the last ply on
 * return, as with gbl_rollout.  A consumer (replay buffer, trainer) reads the trajectory after the launch;
 * between plies nothing but the per-ply outputs touches HBM.
 * ply_dev: NULL, or the device-resident base of the ply index as in gbl_rollout_at. */
int gbl_collect(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                const uint32_t *ply_dev, uint32_t plies, int illegal_mode, int64_t *counters, int32_t *turn,
                void *stream);
/* Trajectory collection with a DEVICE-SIDE POLICY per side (the reference plays whole games with its greedy policy on
 * either or both sides: tutorials/GreedyAgent/tutorial_greedy.py:16-54 -- one GreedyGobbletPolicy object acting for both
 * agents, the first two plies of every game drawn at random -- and gobblet_rl/game/greedy_policy_tianshou.py:63-84,
 * greedy against a learner or a random agent).  gbl_collect with the mover's action chosen inside the launch:
 *   policy0 / policy1  how player_1 / player_2 decide: GBL_POLICY_RANDOM = the masked-uniform draw of gbl_sample
 *                      (generator stream 0, ply index ply0 + t); GBL_POLICY_GREEDY1 / 2 / 3 =
 *                      GreedyGobbletPolicy.compute_action at that depth (greedy_policy.py:38-221; 3 decides like 2, see
 *                      gbl_greedy) on the mover's legal mask and hist[b][mover], and where the reference falls back to
 *                      np.random.choice(actions_depth1) (:211-217) the gbl_sample rule over that candidate set on
 *                      generator stream 1 with the same ply index -- exactly gbl_greedy_act(call = ply0 + t) -- followed
 *                      by the history append of :219.
 *   opening_plies      a greedy side plays the first plies of every game (turn[b] < opening_plies) at random instead,
 *                      without touching its history (tutorial_greedy.py:34-41 uses 2); needs `turn`.  0: none.
 *   hist               int8[n][2][3], read at entry, holds the histories after the last ply on return (they survive a
 *                      game's end, like the reference's policy object); NULL = empty histories, nothing written back.
 * Ply t of board b leaves in cell(t, b) (see gbl_collect) what gbl_greedy_act / gbl_sample + gbl_step with auto-reset would:
 * the seven arrays of gbl_collect, and (each may be NULL)
 *   chosen_traj int32[cells]      gbl_greedy's action_out: the chosen action, -1 where the fallback fired or no greedy
 *                                 policy acted
 *   how_traj    int8 [cells]      GBL_HOW_RANDOM / GBL_HOW_GREEDY / GBL_HOW_FALLBACK: how the action was arrived at
 *   cand_traj   int8 [cells][54]  membership of actions_depth1 at :211 (zeros where no greedy policy acted)
 * Everything else (strides, state / to_move / done / turn / counters at entry and on return, ply_dev) as gbl_collect. */
#define GBL_POLICY_RANDOM 0
#define GBL_POLICY_GREEDY1 1
#define GBL_POLICY_GREEDY2 2
#define GBL_POLICY_GREEDY3 3
#define GBL_HOW_RANDOM 0
#define GBL_HOW_GREEDY 1
#define GBL_HOW_FALLBACK 2
int gbl_collect_policy(int8_t *state, int8_t *to_move, int8_t *done, int8_t *hist, int32_t *actions_traj,
                       int8_t *winner_traj, int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj,
                       int8_t *obs_traj, int32_t *chosen_traj, int8_t *how_traj, int8_t *cand_traj, int64_t n,
                       int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                       const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, int opening_plies,
                       int illegal_mode, int64_t *counters, int32_t *turn, void *stream);

/* Search-driven self-play collection (no counterpart in the reference: the data generator of an AlphaZero-style trainer).
 * gbl_collect with the mover's action chosen inside the launch by a per-side policy, and every ply's search kept:
 *   policy0 / policy1  how player_1 / player_2 decide: GBL_POLICY_RANDOM or GBL_POLICY_TREE.  The greedy policies and flat
 *                      Monte-Carlo are out of scope here (GBL_ERR_ARG); gbl_collect_policy in turn rejects GBL_POLICY_TREE.
 * Per board g = env_base + b, for t = 0 .. plies-1, ply index q = ply0 + t (+ *ply_dev), mover m:
 *   RANDOM  the gbl_sample rule on generator stream 0 with ply index q, exactly as gbl_collect.
 *   TREE    the search is exactly gbl_tree_search(state, to_move, mask = NULL, iterations_m, playouts_m, max_plies, explore, seed,
 *           env_base, call = q) of the board's current position (the same rule text, the same draws on stream 3), and the action
 *           is that search's action_out -- except while turn[b] < sample_plies, where the action is drawn in proportion to the
 *           visits: S = the sum of visits_out, r = the generator word of (seed, g, q, stream 4), k = (r * S) >> 32, and the
 *           lowest action whose running sum of visits exceeds k.  sample_plies > 0 needs `turn`.  A root without a candidate gives
 *           action -1, which is stepped as gbl_step steps an illegal action (per illegal_mode).
 *   then    gbl_step with auto-reset and illegal_mode, as in gbl_collect.
 * Ply t of board b leaves in cell(t, b) (see gbl_collect; both layouts) the seven arrays of gbl_collect, and (every pointer may be NULL)
 *   visits_traj int16[cells][54]  visits_out of the search that chose the action of ply t; zeros where RANDOM moved
 *   value_traj  int32[cells]      the sum over the actions of wins_out - losses_out of that search, from the mover's side (the games
 *                                 behind it: S * playouts_m); 0 where RANDOM moved
 *   nodes_traj  int32[cells]      that search's nodes_out; 0 where RANDOM moved
 *   how_traj    int8 [cells]      GBL_HOW_RANDOM, GBL_HOW_SEARCH (the search's decision) or GBL_HOW_SEARCH_SAMPLED (the draw)
 *   mover_traj  int8 [cells]      the agent who played ply t
 * The limits of iterations / playouts / max_plies / explore / env_base are those of gbl_tree_search (a RANDOM side's pair is
 * ignored), sample_plies >= 0, and ply0 + plies <= 2^24 because `call` has 24 bits (with ply_dev the caller
 * keeps the sum below it).  state / to_move / done / turn / counters / ply_dev and the strides as gbl_collect; the state rows are
 * rebuilt from bit planes on return (see the contract on `state` above).  Allocates nothing; the tree lives in
 * 16 (max(iterations0, iterations1) + 1) bytes of LDS per workgroup and is rebuilt from an empty root on every ply. */
#define GBL_POLICY_TREE 4
#define GBL_HOW_SEARCH 3
#define GBL_HOW_SEARCH_SAMPLED 4
int gbl_collect_search(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                       int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                       int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                       int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                       const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, int iterations0, int iterations1,
                       int playouts0, int playouts1, int max_plies, int explore, int sample_plies, int illegal_mode,
                       int64_t *counters, int32_t *turn, void *stream);

/* Evaluator-guided self-play collection (no counterpart in the reference): gbl_collect_search with gbl_tree_search_eval in place of
 * the playout search -- the step an AlphaZero-style loop repeats, and, with two different networks, the arena that gates a new one.
 *   policy0 / policy1  how player_1 / player_2 decide: GBL_POLICY_RANDOM or GBL_POLICY_EVAL_TREE.  GBL_POLICY_TREE and the greedy
 *                      policies are out of scope here (GBL_ERR_ARG); gbl_collect_policy and gbl_collect_search in turn reject
 *                      GBL_POLICY_EVAL_TREE.
 *   ev0 / ev1          the networks of player_1 / player_2 (gbl_evaluator, above).  They may be the same struct and may have different
 *                      `hidden`; NULL is allowed only for a RANDOM side.
 * Per board g = env_base + b, for t = 0 .. plies-1, ply index q = ply0 + t (+ *ply_dev), mover m:
 *   RANDOM     the gbl_sample rule on generator stream 0 with ply index q, exactly as gbl_collect_search.
 *   EVAL_TREE  the search is exactly gbl_tree_search_eval(state, to_move, mask = NULL, ev_m, iterations_m, explore) of the board's
 *              current position, and the action is that search's action_out -- except while turn[b] < sample_plies, where the action
 *              is drawn in proportion to the visits by gbl_collect_search's rule: S = the sum of visits_out, r = the generator word of
 *              (seed, g, q, stream 4), k = (r * S) >> 32, and the lowest action whose running sum of visits exceeds k.  The search
 *              itself still draws nothing: seed, env_base and q matter only for RANDOM sides and that draw.  A root without a
 *              candidate gives action -1, which is stepped as gbl_step steps an illegal action (per illegal_mode).
 *   then       gbl_step with auto-reset and illegal_mode, as in gbl_collect.
 * Ply t of board b leaves in cell(t, b) (see gbl_collect; both layouts) the seven arrays of gbl_collect, and (every pointer may be NULL)
 *   visits_traj     int16[cells][54]  visits_out of the search that chose the action of ply t; zeros where RANDOM moved
 *   value_traj      int32[cells]      the sum over the actions of wins_out - losses_out of that search, in 1/128 of a game, from the
 *                                     mover's side; 0 where RANDOM moved
 *   nodes_traj      int32[cells]      that search's nodes_out; 0 where RANDOM moved
 *   how_traj        int8 [cells]      GBL_HOW_RANDOM, GBL_HOW_SEARCH or GBL_HOW_SEARCH_SAMPLED
 *   mover_traj      int8 [cells]      the agent who played ply t
 *   root_value_traj int32[cells]      that search's root_value_out (written also for a root without a candidate); 0 where RANDOM moved
 *   priors_traj     uint8[cells][54]  that search's root_priors_out; zeros where RANDOM moved
 * 1 <= iterations <= 512, 0 <= explore <= 1024 and the evaluator's rules are those of gbl_tree_search_eval (a RANDOM side's evaluator
 * and iterations are ignored), sample_plies >= 0 (> 0 needs `turn`), ply0 + plies <= 2^24 and env_base + n <= 2^42 as
 * gbl_collect_search.  state / to_move / done / turn / counters / ply_dev, the strides and the alignment rules as gbl_collect_search
 * (root_value_traj 4-byte aligned; priors_traj needs none); the state rows are rebuilt from bit planes on return.  gbl_outcome_targets
 * works on these trajectories unchanged.  Allocates nothing; the tree lives in 72 (max(iterations of the searching sides) + 1) bytes of
 * LDS per workgroup and is rebuilt from an empty root on every ply: nothing persists from one ply's search to the next. */
#define GBL_POLICY_EVAL_TREE 5
int gbl_collect_search_eval(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                            int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                            int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                            int32_t *root_value_traj, uint8_t *priors_traj, int64_t n, int64_t ply_stride, int64_t tile_stride,
                            uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int policy0,
                            int policy1, const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0, int iterations1,
                            int explore, int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn, void *stream);

/* Solver-guarded evaluator self-play (no counterpart in the reference): gbl_collect_search_eval with gbl_solve in front of every
 * search, inside the same launch -- a side that is guarded never passes over a win the solver proves and never steps into a loss it
 * proves beside an unproven move.  Everything is as gbl_collect_search_eval (policies GBL_POLICY_RANDOM / GBL_POLICY_EVAL_TREE, ev0 /
 * ev1, the window, the strides, the twelve arrays and root_value_traj / priors_traj), with
 *   solve_depth0 / solve_depth1  the guard's depth for player_1 / player_2: 0 = no guard, else 1 .. GBL_SOLVE_MAX_DEPTH.  A RANDOM
 *                                side's depth is ignored, as its evaluator and iterations are.
 * The one exception to gbl_collect_search_eval's rule is the ply of a mover m with policy EVAL_TREE and solve_depth_m = d > 0:
 *   solve     (outcome, V, a*) = gbl_solve(state, to_move, mask = NULL, depth = d) of the board's current position: the same rule text.
 *   proven    V != 0 (the root holds a forced win, or every candidate is a forced loss): the action is a* -- the shortest win, else
 *             the longest loss, the lowest index on ties.  No search runs and nothing is drawn, also while turn[b] < sample_plies.
 *             how = GBL_HOW_PROVEN; the visits row holds iterations_m at a* and 0 elsewhere (visits / sum is one-hot, and
 *             gbl_training_batch keeps the ply); value = sign(V) * 128 * iterations_m; nodes = 0, root_value = 0, the prior row zeros.
 *   unproven  V == 0 and at least one outcome is 0.  With C = the actions whose outcome is 0, the search is exactly
 *             gbl_tree_search_eval(state, to_move, mask = C, ev_m, iterations_m, explore); the action is its action_out or, while
 *             turn[b] < sample_plies, the visit-proportional draw on stream 4; how, visits, value, nodes, root_value and priors are
 *             what gbl_collect_search_eval writes for that search.
 *   a root without a candidate: as EVAL_TREE in gbl_collect_search_eval (action -1, stepped per illegal_mode).
 * Two more arrays per cell (either may be NULL):
 *   outcome_traj int8[cells][54]  the solver's outcome_out row of ply t's position
 *   proven_traj  int8[cells]      the solver's V
 * On plies of a RANDOM side, of a side with depth 0 and of a root without a candidate the outcome row is all GBL_SOLVE_NONE and V is 0.
 * With both depths 0 every shared array is that of gbl_collect_search_eval, bit for bit.  A depth outside 0 .. GBL_SOLVE_MAX_DEPTH on
 * an EVAL_TREE side is GBL_ERR_ARG; every other limit, the alignment rules (outcome_traj / proven_traj need none) and the LDS of the
 * tree as gbl_collect_search_eval, beside which the solver keeps 872 bytes.  gbl_outcome_targets and gbl_training_batch work on these
 * trajectories unchanged.  Allocates nothing. */
#define GBL_HOW_PROVEN 5
int gbl_collect_search_solve(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                             int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                             int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                             int32_t *root_value_traj, uint8_t *priors_traj, int8_t *outcome_traj, int8_t *proven_traj, int64_t n,
                             int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                             const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0,
                             const gbl_evaluator *ev1, int iterations0, int iterations1, int solve_depth0, int solve_depth1, int explore,
                             int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn, void *stream);

/* Self-play with root noise: gbl_collect_search_solve with one noise weight per side, noise0 / noise1 in 0 .. 256 for player_1 /
 * player_2.  A side's weight is ignored unless that side is EVAL_TREE.  The ply q of a mover m is gbl_collect_search_solve's text with
 * the search replaced by gbl_tree_search_eval_noise(..., noise_m, seed, env_base, call = q) over the same candidate set: the legal
 * mask where the side is unguarded, the actions of outcome 0 where it is guarded.  A proven ply searches nothing and draws nothing.
 * The arrays are gbl_collect_search_solve's; priors_traj stays the network's row pi (nu is a function of (seed, g, q, C): a consumer
 * recomputes it).  With both weights 0 every array is gbl_collect_search_solve's, bit for bit.  The noise moves with *ply_dev as every
 * other draw of the window does.  A weight outside 0 .. 256 on an EVAL_TREE side is GBL_ERR_ARG; everything else as
 * gbl_collect_search_solve.  Allocates nothing. */
int gbl_collect_search_noise(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                             int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                             int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                             int32_t *root_value_traj, uint8_t *priors_traj, int8_t *outcome_traj, int8_t *proven_traj, int64_t n,
                             int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                             const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0,
                             const gbl_evaluator *ev1, int iterations0, int iterations1, int solve_depth0, int solve_depth1, int noise0,
                             int noise1, int explore, int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn, void *stream);

/* Self-play with playout-cap randomisation (no counterpart in the reference): gbl_collect_search_noise with a random share of an
 * EVAL_TREE side's plies searched in full and the rest played from a small search that leaves no policy target.
 *   full_share0 / full_share1          the share of full plies of player_1 / player_2, in 0 .. 256, in 1/256: 256 = every ply is full,
 *                                      0 = every ply is fast
 *   fast_iterations0 / fast_iterations1  the budget of a fast ply, 1 <= fast_iterations_m <= iterations_m (the LDS tree stays sized
 *                                      by iterations)
 * Both are read only for an EVAL_TREE side, and fast_iterations_m only where full_share_m < 256.  The rule is
 * gbl_collect_search_noise's text with one addition, for ply q of an EVAL_TREE mover m with full_share_m < 256 on board
 * g = env_base + b:
 *   draw      r = the generator word of (seed, g, ply index q, stream 9) -- gbl_sample's generator: counter (g_lo, g_hi, q >> 2, 9),
 *             word q & 3; stream 9 is the cap's own.  The ply is FULL iff (r >> 24) < full_share_m.  The draw moves with *ply_dev as
 *             every other draw of the window does.
 *   full ply  exactly gbl_collect_search_noise's ply.
 *   fast ply  the solver guard runs as before; a proven root is gbl_collect_search_solve's proven ply, unchanged (GBL_HOW_PROVEN, the
 *             one-hot row at iterations_m, nothing drawn).  Otherwise the search is exactly gbl_tree_search_eval(state, to_move,
 *             mask = C, ev_m, fast_iterations_m, explore) -- no noise -- with C the legal mask, or the actions of outcome 0 under a
 *             guard.  The action is its action_out or, while turn[b] < sample_plies, the visit-proportional draw on stream 4 over that
 *             search's visits.  how = GBL_HOW_FAST or GBL_HOW_FAST_SAMPLED; the visits row holds 54 ZEROS (gbl_training_batch,
 *             gbl_replay_append and gbl_train_step drop the cell: a fast ply is no policy target); value, nodes, root_value and
 *             priors are what that search wrote; outcome / proven as on a full ply.
 *   a root without a candidate behaves as before.
 * With both shares 256 every array is gbl_collect_search_noise's, bit for bit.  A board's window depends on (seed, g, the ply
 * indices) alone, not on the batch or the shard.  Errors are gbl_collect_search_noise's in its order; after its noise check comes
 * GBL_ERR_ARG for a share outside 0 .. 256 on an EVAL_TREE side, then for a fast_iterations outside 1 .. iterations_m where it is
 * read.  gbl_outcome_targets, gbl_training_batch and gbl_replay_append work on these trajectories unchanged.  Allocates nothing. */
#define GBL_HOW_FAST 8
#define GBL_HOW_FAST_SAMPLED 9
int gbl_collect_search_cap(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                           int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                           int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                           int32_t *root_value_traj, uint8_t *priors_traj, int8_t *outcome_traj, int8_t *proven_traj, int64_t n,
                           int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                           const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0,
                           const gbl_evaluator *ev1, int iterations0, int iterations1, int solve_depth0, int solve_depth1, int noise0,
                           int noise1, int explore, int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn,
                           int fast_iterations0, int fast_iterations1, int full_share0, int full_share1, void *stream);

/* Self-play with the Gumbel root search: gbl_collect_search_eval with one `considered` per side, considered0 / considered1 in 0 .. 54
 * for player_1 / player_2, and gumbel_noise / visit_offset / scale for both.  A side's value is ignored unless that side is EVAL_TREE;
 * considered_m == 0 means that side searches exactly as in gbl_collect_search_eval, and with both 0 every array is
 * gbl_collect_search_eval's, bit for bit (gumbel_noise, visit_offset and scale are then not read).  The ply q of an EVAL_TREE mover m
 * with considered_m > 0 is
 *   search   gbl_tree_search_gumbel(state, to_move, mask = NULL, ev_m, iterations_m, explore, considered_m, gumbel_noise,
 *            visit_offset, scale, seed, env_base, call = q) of the board's current position.
 *   action   that search's action_out.  sample_plies is not read for this side: the Gumbel row is its exploration.
 *   how      GBL_HOW_GUMBEL.
 *   visits   visits_traj holds the TARGET row target_out, an int16 in 1 .. 255 on C and 0 elsewhere: gbl_outcome_targets,
 *            gbl_training_batch, gbl_replay_append and gbl_train_step read it unchanged as visits / sum.
 *   value, nodes, root_value and priors are what gbl_collect_search_eval writes for a search (value from the raw wins and losses).
 *   a root without a candidate: action -1, stepped per illegal_mode, the row zeros, how = GBL_HOW_GUMBEL.
 * The Gumbel row moves with *ply_dev as every other draw of the window does; a consumer recomputes it from (seed, g, q).  Errors are
 * gbl_collect_search_eval's in its order; after them (before the n == 0 return) GBL_ERR_ARG for a considered outside 0 .. 54 on an
 * EVAL_TREE side, then, where a side follows the rule, for gumbel_noise, visit_offset, scale out of range.  The solver guard goes
 * with the rule in gbl_collect_gumbel_solve, below, and the tablebase in gbl_collect_gumbel_tb; root noise and the playout cap are not
 * combined with it.  Allocates nothing; the LDS is gbl_collect_search_eval's. */
#define GBL_HOW_GUMBEL 10
int gbl_collect_search_gumbel(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                              int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                              int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                              int32_t *root_value_traj, uint8_t *priors_traj, int64_t n, int64_t ply_stride, int64_t tile_stride,
                              uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int policy0,
                              int policy1, const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0, int iterations1,
                              int explore, int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn, int considered0,
                              int considered1, int gumbel_noise, int visit_offset, int scale, void *stream);

/* Solver-guarded Gumbel self-play (no counterpart in the reference): gbl_collect_search_solve with the unproven ply's search replaced
 * by the Gumbel root search, inside the same launch.  The arguments are gbl_collect_search_solve's, followed by
 * gbl_collect_search_gumbel's five: considered0 / considered1 in 0 .. 54 for player_1 / player_2, and gumbel_noise / visit_offset /
 * scale for both.  A side's depth and `considered` are ignored unless that side is EVAL_TREE.  The ply q of an EVAL_TREE mover m on
 * board g = env_base + b:
 *   solve_depth_m = d > 0 and the root has a candidate: (outcome, V, a*) = gbl_solve(state, to_move, mask = NULL, depth = d) of the
 *   board's current position, as in gbl_collect_search_solve.
 *     proven    V != 0: exactly gbl_collect_search_solve's proven ply -- the action is a*, how = GBL_HOW_PROVEN, the visits row holds
 *               iterations_m at a* and 0 elsewhere, value = sign(V) * 128 * iterations_m, nodes = 0, root_value = 0, the prior row
 *               zeros.  No search runs, nothing is drawn and no Gumbel row is made.
 *     unproven  V == 0.  With C = the actions whose outcome is 0:
 *               considered_m > 0   the search is gbl_tree_search_gumbel(state, to_move, mask = C, ev_m, iterations_m, explore,
 *                                  considered_m, gumbel_noise, visit_offset, scale, seed, env_base, call = q): the rule considers
 *                                  min(considered_m, |C|) actions of C.  The action is its action_out, how = GBL_HOW_GUMBEL, and
 *                                  visits_traj holds its target_out -- 1 .. 255 on C, 0 elsewhere; value, nodes, root_value and priors
 *                                  as gbl_collect_search_gumbel writes them.  sample_plies is not read for this side.
 *               considered_m == 0  gbl_collect_search_solve's unproven ply: gbl_tree_search_eval(mask = C), the visit-proportional
 *                                  draw while turn[b] < sample_plies.
 *   solve_depth_m == 0: the side's ply is gbl_collect_search_gumbel's (over the legal mask); the outcome row is all GBL_SOLVE_NONE
 *   and V is 0.
 *   RANDOM sides, a root without a candidate, *ply_dev, the strides, counters and turn: as in gbl_collect_search_solve and
 *   gbl_collect_search_gumbel, which agree on them.
 * With both depths 0 every shared array is gbl_collect_search_gumbel's, bit for bit; with both `considered` 0 every array is
 * gbl_collect_search_solve's, bit for bit.  A board's window depends on (seed, g, the ply indices) alone.  Errors are
 * gbl_collect_search_solve's in its order (a depth outside 0 .. GBL_SOLVE_MAX_DEPTH on an EVAL_TREE side among them); after them,
 * before the n == 0 return, GBL_ERR_ARG for a considered outside 0 .. 54 on an EVAL_TREE side, then, where a side follows the rule,
 * for gumbel_noise, visit_offset, scale out of range; then the pointers.  Root noise and the playout cap are not combined with
 * the rule; the tablebase is in gbl_collect_gumbel_tb, without the guard.  gbl_outcome_targets, gbl_training_batch and gbl_replay_append work on these trajectories unchanged.
 * Allocates nothing; the LDS is gbl_collect_search_solve's: the tree and the solver's 872 bytes. */
int gbl_collect_gumbel_solve(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                             int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                             int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                             int32_t *root_value_traj, uint8_t *priors_traj, int8_t *outcome_traj, int8_t *proven_traj, int64_t n,
                             int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                             const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0,
                             const gbl_evaluator *ev1, int iterations0, int iterations1, int solve_depth0, int solve_depth1, int explore,
                             int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn, int considered0, int considered1,
                             int gumbel_noise, int visit_offset, int scale, void *stream);

/* Outcome targets of a collected window of `plies` plies (the value target of a position is the result of the game it belongs
 * to).  For cell (t, b), with e the smallest t' >= t whose done_traj[cell(t', b)] is non-zero:
 *   z_traj          int8 [cells]  reward_traj[cell(e, b)][mover_traj[cell(t, b)]] -- the reward, not the winner, so that
 *                                 GBL_ILLEGAL_TERMINATE's -1 comes out right; GBL_Z_OPEN where no game end lies in the window
 *   plies_left_traj int16[cells]  e - t, or -1 where no game end lies in the window (may be NULL)
 * done_traj / reward_traj / mover_traj / z_traj are required; strides and cells as gbl_collect; plies <= 32767. */
#define GBL_Z_OPEN (-128)
int gbl_outcome_targets(const int8_t *done_traj, const int8_t *reward_traj, const int8_t *mover_traj, int8_t *z_traj,
                        int16_t *plies_left_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint32_t plies, void *stream);

/* Board symmetries (no counterpart in the reference: the augmentation step of an AlphaZero-style trainer).  A symmetry is an integer
 * s in [0, GBL_SYMMETRIES): one of the 8 symmetries of the square acting on the 9 positions, times the exchange of the two equal-sized
 * pieces of a colour (piece numbers 2k+1 <-> 2k+2), three independent swaps per colour: 8 x 8 x 8 = 512 elements.
 *   Position map sigma.  Bits 0-1 = rot, bit 2 = flip.  For the cell (r, c) of position p = 3 r + c: if flip, c <- 2 - c; then rot
 *     times (r, c) <- (c, 2 - r).  sigma(p) = 3 r + c of the result: the position a piece on p moves to.
 *   Piece swaps.  Bit 3 + k (k = 0, 1, 2) swaps player_1's pieces 2k+1 <-> 2k+2, bit 6 + k those of player_2.  tau_m is the resulting
 *     map on agent m's piece numbers 1..6 (m = 0: player_1).
 *   State row (27 B).  out[9 l + sigma(p)] = sign(v) * tau_m(|v|) for v = in[9 l + p] with |v| in 1..6, m the owner (v > 0: player_1);
 *     every other byte value (0, and what no contract state holds) is moved unchanged.
 *   An action of agent m.  a = 9 (piece - 1) + p  |->  A_m(a) = 9 (tau_m(piece) - 1) + sigma(p); actions outside [0, 54) pass unchanged.
 *   Action-indexed rows (mask int8[54], visits int16[54], priors uint8[54]; candidate sets and solver outcomes are such rows too):
 *     out[A_m(a)] = in[a].
 *   Observation row (117 B, byte 13 p + ch) as seen by agent m: channels 0-5 (the viewer's pieces, channel = piece - 1) are permuted by
 *     tau_m, channels 6-11 (the other side's) by tau_(1-m), channel 12 stays; cells move by sigma.
 *   z, values, rewards, winners and done do not change.
 * What is symmetric.  The legal mask, the observation and a step commute with every element.  The piece swaps are symmetries of
 * check_for_winner() everywhere.  The square's symmetries are too, EXCEPT on boards where both colours hold a line at once (a lift
 * uncovered the other side's line): there the reference's "last matching line decides" (board.py:183-194) makes the order of the
 * lines count, and a reflection or rotation changes that order.  Such boards are about 0.04 % of masked-random play.
 *
 * gbl_symmetry_apply: for n boards, the image under sym[b] (const int16_t[n]; only its low 9 bits are read) of whichever rows are
 * given -- or under sym_all, in [0, 512), for every board when sym is NULL.  Every _in / _out pair is optional (both NULL) but goes
 * together; agent (int8[n], non-zero = player_2: whose view / whose actions) is required as soon as anything but the state pair is
 * given.  The transform is a permutation and NOT in-place safe: an _out equal to its _in is GBL_ERR_ARG.  state / obs / mask /
 * visits / priors buffers must be 16-byte aligned, actions 4-byte aligned (GBL_ERR_ALIGN).  One launch; allocates nothing. */
#define GBL_SYMMETRIES 512
int gbl_symmetry_apply(const int16_t *sym, int sym_all, const int8_t *agent, const int8_t *state_in, int8_t *state_out,
                       const int8_t *obs_in, int8_t *obs_out, const int8_t *mask_in, int8_t *mask_out, const int16_t *visits_in,
                       int16_t *visits_out, const uint8_t *priors_in, uint8_t *priors_out, const int32_t *actions_in,
                       int32_t *actions_out, int64_t n, void *stream);

/* Symmetry-augmented training batches drawn on the device from a collected window with outcome targets (gbl_collect_search /
 * gbl_collect_search_eval + gbl_outcome_targets; strides and cell(t, b) as gbl_collect, both layouts).
 *   Valid cells.  Cell (t, b), 1 <= t < plies, is valid iff z_traj[cell(t, b)] != GBL_Z_OPEN, done_traj[cell(t - 1, b)] == 0 (slot
 *     t - 1 holds what the mover of ply t saw, unless a game ended there) and the 54 visits of cell(t, b) sum to more than 0.
 *   Draw of sample j (j = 0 .. batch - 1).  For attempt i = 0 .. GBL_BATCH_ATTEMPTS - 1: (w0, w1, w2, w3) = the block
 *     Philox4x32-10(ctr = (id_lo, id_hi, 16 call + i, 5), key = (seed_lo, seed_hi)) with id = sample_base + j -- the gbl_sample
 *     generator with ply index 4 (16 call + i) + w on stream 5 --, t = 1 + ((w0 * (plies - 1)) >> 32), b = (w1 * n) >> 32.  The first
 *     attempt whose cell (t, b) is valid is taken; its symmetry is s = w2 & sym_mask (sym_mask in [0, 511]: 0 = none, 7 = the square
 *     only, 511 = the whole group).  The draw of sample j depends on (seed, sample_base + j, call) alone: not on batch, not on the
 *     launch.  call < 2^26.  A sample is not exactly uniform over the valid cells of a window only in that it may fail: with a valid
 *     share v of the cells, with probability (1 - v)^16.
 *   Outputs, row j (all optional but index_out), with m = mover_traj[cell(t, b)] != 0 the agent:
 *     obs_out    int8 [batch][117] the image of obs_traj[cell(t - 1, b)]       (needs obs_traj)
 *     mask_out   int8 [batch][54]  the image of mask_traj[cell(t - 1, b)]      (needs mask_traj)
 *     visits_out int16[batch][54]  the image of visits_traj[cell(t, b)]
 *     z_out      int8 [batch]      z_traj[cell(t, b)]
 *     index_out  int32[batch][2]   (t, b)                    sym_out int16[batch]  s
 *     A sample without a valid attempt: zero rows, z = GBL_Z_OPEN, index (-1, -1), sym 0.
 * Argument errors: plies < 2 or > 32767, batch < 0 or > 2^31, sym_mask outside [0, 511], call >= 2^26, and with batch > 0: n < 1 or n > 2^31,
 * a missing required pointer, and gbl_collect's stride rules.  batch == 0 returns GBL_OK after the scalar checks.  visits_traj and
 * index_out must be 4-byte aligned, sym_out 2-byte, obs_out / mask_out / visits_out 16-byte (GBL_ERR_ALIGN); the window's byte arrays
 * need no alignment.  One launch, one wavefront per 64 samples; allocates nothing, no atomics. */
#define GBL_BATCH_ATTEMPTS 16
int gbl_training_batch(const int8_t *obs_traj, const int8_t *mask_traj, const int16_t *visits_traj, const int8_t *z_traj,
                       const int8_t *done_traj, const int8_t *mover_traj, int64_t n, uint32_t plies, int64_t ply_stride,
                       int64_t tile_stride, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base, uint32_t call,
                       int8_t *obs_out, int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out, int16_t *sym_out,
                       void *stream);

/* One Adam step of the FLOAT network that GobbletEvaluator.from_float quantises (no counterpart in the reference), on a batch shaped
 * as gbl_training_batch writes it:  h = relu(x w1 + b1),  o = h w2 + b2.  The rule is BIT-DEFINED: every operation below is ONE
 * IEEE-754 binary32 multiply, add, subtract, divide or square root, correctly rounded (no fused multiply-add, no reciprocal or
 * rsqrt approximation, denormals kept), in the order written, so that the kernels, the host flavour and a numpy-float32 restatement
 * of this text agree bit for bit.  Two launches, no atomics, allocates nothing.
 *   Inputs.  obs int8 [B][117], a byte counts as 1 wherever it is non-zero; mask int8 [B][54] (NULL: all 54 actions), C_r = {a :
 *     mask[r][a] != 0}; visits int16 [B][54]; z int8 [B].  1 <= B <= 65 536.  S_r = the integer sum of visits[r][a] over C_r.  Row r
 *     COUNTS iff z[r] != GBL_Z_OPEN and S_r > 0 (a sample gbl_training_batch could not draw counts for nothing).  An uncounted row
 *     has h = dh = do = 0 and both loss terms 0 below.  N = the number of counted rows, M = max(N, 1) as a float.
 *   Parameters.  params float [P], P = 117 H + H + 55 H + 55, in the order w1[117][H], b1[H], w2[H][55], b2[55] (from_float's
 *     shapes); adam_m and adam_v float [P] alike.  H is 64, 128, 192 or 256.
 *   Forward of a counted row (ascending means: an accumulator that starts with the first value named and takes one add per term).
 *     pre_j = b1_j, then + w1[f][j] for every f with x_f = 1, f ascending            h_j = pre_j > 0 ? pre_j : 0
 *     o_k   = b2_k, then + h_j * w2[j][k] for j = 0 .. H - 1 ascending               k = 0 .. 54
 *     mx    = o_a of the first a in C, then for the other a in C ascending: mx = o_a > mx ? o_a : mx
 *     d_a   = o_a - mx,  e_a = EXP(d_a)  (a in C);   s = 0, then + e_a for a in C ascending;   L = LOG(s)
 *     t_a   = float(visits_a) / float(S),  p_a = e_a / s
 *     policy loss  lp = 0, then + t_a * (L - d_a) for a in C ascending               (the log-sum form of -sum t log p)
 *     v = o_54,  c = v < -1 ? -1 : (v > 1 ? 1 : v),  u = c - float(z)
 *     value loss   lv = u * u + value_reg * (v * v)
 *   Backward.  do_a = p_a - t_a (a in C), 0 for the other a < 54;  do_54 = 2 * (-1 < v < 1 ? u : 0) + 2 * (value_reg * v);
 *     dh_j = pre_j > 0 ? (0, then + do_k * w2[j][k] for k = 0 .. 54 ascending) : 0.
 *   Row sums.  Rows are summed in CHUNKS of 64: chunk c holds rows 64 c .. min(64 c + 63, B - 1).  SUM(term) = 0, then + the chunk
 *     sums for c ascending, each chunk sum = 0, then + term_r for its rows ascending.
 *       G(w1[f][j]) = SUM(dh_j of the rows with x_f = 1; the other rows add nothing)     G(b1_j) = SUM(dh_j)
 *       G(w2[j][k]) = SUM(h_j * do_k)                                                    G(b2_k) = SUM(do_k)
 *     gradient  g = G / M + weight_decay * theta        (torch Adam's L2 form)
 *   Adam, per element, with hy = *hyper:
 *     m' = beta1 * m + (1 - beta1) * g        v' = beta2 * v + (1 - beta2) * (g * g)        (1 - beta is one float subtraction)
 *     theta' = theta - (lr * (m' / bias1)) / (sqrt(v' / bias2) + eps)
 *     The caller computes bias1 = 1 - beta1^t and bias2 = 1 - beta2^t (t = 1, 2, ... the step) in double and passes them as floats.
 *   EXP(x), x <= 0:  x = max(x, -110);  n = int(x * LOG2E - 0.5) (the cast truncates);  r = (x - n * LN2_HI) - n * LN2_LO;
 *     q = C7, then q = q * r + C_i for i = 6 .. 2 (two operations each);  y = ((r * r) * q + r) + 1;  n1 = n >> 1, n2 = n - n1;
 *     EXP = (y * 2^n1) * 2^n2, the powers of two built from their exponent bits.  LOG2E = 0x1.715476p+0, LN2_HI = 0x1.62e4p-1,
 *     LN2_LO = 0x1.7f7d1cp-20, C2 .. C7 = 0x1p-1 0x1.555556p-3 0x1.555556p-5 0x1.111112p-7 0x1.6c16c2p-10 0x1.a01a02p-13.
 *   LOG(s), s >= 1 (here s <= 54):  s = 2^e * w with the mantissa w in [1, 2); if w's 23 mantissa bits exceed 0x3504f3 (sqrt 2)
 *     then w = w / 2, e = e + 1 (on the bits);  f = w - 1,  q = f / (2 + f),  y = q * q;
 *     R = D4, then R = R * y + D_i for i = 3 .. 1, then R = R * y;  hf = (0.5 * f) * f;  T = q * (hf + R);
 *     LOG = (((T + e * LN2_LO) - hf) + f) + e * LN2_HI.  D1 .. D4 = 0x1.555556p-1 0x1.99999ap-2 0x1.24924ap-2 0x1.c71c72p-3.
 *     (Measured over 2^20 evenly spaced arguments and the range edges, and asserted as the bound by tests/test_train_step.py:
 *      EXP is within 0.99491 ulp on [-104, 0], LOG within 0.74746 ulp on [1, 54].)
 *   Outputs.  params, adam_m, adam_v updated in place; grad_out float [P] (may be NULL): g;  stats_out float [4]: SUM(lp) / M,
 *     SUM(lv) / M, float(N), and the largest h_j over the counted rows (0 without one: what from_float takes as hidden_max).
 *   Workspace.  The caller supplies gbl_train_workspace_bytes bytes (4 B (2 H + 60); it holds h, dh, do and the loss terms of
 *     every row between the two launches); that function returns 0 for a batch or hidden out of range and launches nothing.
 * Argument errors (GBL_ERR_ARG): hidden or batch out of range, a missing pointer (all but mask and grad_out are required), a
 * workspace_bytes that is too small.  GBL_ERR_ALIGN: obs, mask, visits, the float arrays and the workspace must be 16-byte
 * aligned (the host flavour asks no alignment). */
typedef struct {
    float lr, beta1, beta2, eps, weight_decay, value_reg, bias1, bias2;
} gbl_train_hyper;
int64_t gbl_train_workspace_bytes(int64_t batch, int hidden);
int gbl_train_step(const int8_t *obs, const int8_t *mask, const int16_t *visits, const int8_t *z, int64_t batch, int hidden,
                   float *params, float *adam_m, float *adam_v, const gbl_train_hyper *hyper, float *grad_out, float *stats_out,
                   void *workspace, int64_t workspace_bytes, void *stream);

/* gbl_train_step with a weight per row, and with the rows' own losses handed out: the step of a prioritised fit (a row drawn with
 * probability priority / W counts with its importance weight, and its loss becomes its next priority).  Everything is gbl_train_step's --
 * inputs, parameters, workspace, stats_out's layout, the two launches, every operation ONE binary32 operation in the order written -- with
 * these additions:
 *   row_weight float [B] (NULL: every weight is 1).  The effective weight  ww_r = (row_weight[r] > 0 && row_weight[r] <= FLT_MAX) ?
 *     row_weight[r] : 0  -- a NaN, a negative, a zero and +inf all count 0.
 *   Which rows count, N and M = max(N, 1) are UNCHANGED: a row of weight 0 still counts in N and in the hidden maximum (the "mean of
 *     w * loss over the batch" form).
 *   Forward, lp, lv and do_k of a counted row as above.  Then  do'_k = ww_r * do_k  for k = 0 .. 54, one multiply each; do' takes do's
 *     place: dh_j is formed from do', G(w2[j][k]) = SUM(h_j * do'_k), G(b2_k) = SUM(do'_k).  The row's loss terms enter their sums as
 *     ww_r * lp and ww_r * lv (one multiply each), so stats_out = SUM(ww lp) / M, SUM(ww lv) / M, float(N), the hidden maximum.
 *   row_loss_out float [B][2] (may be NULL): (lp, lv) UNWEIGHTED; (0, 0) for an uncounted row.
 *   prio_out int32 [B] (may be NULL): 0 for an uncounted row; otherwise  q = (lp + lv) * prio_scale (one add, then one multiply);
 *     k = 0 if !(q > 0), k = 2^30 if q >= 0x1p30, else k = (int32)q (the cast truncates);  prio_out = min((int64)prio_floor + k, prio_cap).
 *     The map is linear in the loss.  prio_scale, prio_floor and prio_cap are read only when prio_out is given.
 *   By construction: with row_weight NULL or every weight exactly 1.0f all five outputs of gbl_train_step come out bit for bit (1.0f * x
 *     is x, denormals included), and row_loss_out and prio_out do not depend on the weights.
 * Errors: gbl_train_step's in its order (alignment rules included); then GBL_ERR_ARG unless prio_scale is finite and >= 0, GBL_ERR_ARG
 * unless 0 <= prio_floor <= prio_cap (both only with prio_out); then GBL_ERR_ALIGN unless row_weight, row_loss_out and prio_out are
 * 4-byte aligned (device flavour only).
 * The rows kernel is a second instantiation of gbl_train_step's (the weight sits in a scalar register and is folded into the stores of
 * do and of the loss terms; the two outputs are written by the lanes that hold lp and lv: no third launch, no atomics); the second
 * launch is gbl_train_step's own.  Measured: DESIGN.md 5.24, profiles/r26/train_weighted.json. */
int gbl_train_step_weighted(const int8_t *obs, const int8_t *mask, const int16_t *visits, const int8_t *z, int64_t batch, int hidden,
                            float *params, float *adam_m, float *adam_v, const gbl_train_hyper *hyper, const float *row_weight,
                            float *row_loss_out, int32_t *prio_out, float prio_scale, int32_t prio_floor, int32_t prio_cap, float *grad_out,
                            float *stats_out, void *workspace, int64_t workspace_bytes, void *stream);

/* Replay buffer (no counterpart in the reference: the memory of an AlphaZero-style loop across collected windows).  A ring of
 * `capacity` compacted training rows in device memory, 1 <= capacity <= 2^31 - 1, in three arrays whose rows are whole 128-byte
 * lines (or half of one), so that a drawn row costs one line per array:
 *   ring_obs    int8 [capacity][GBL_REPLAY_OBS_PITCH]     bytes 0 .. 116: obs_traj[cell(t - 1, b)], what the mover saw; 117 .. 127: zero.
 *                                                         Optional: NULL is a buffer without observations.
 *   ring_visits int16[capacity][GBL_REPLAY_VISITS_PITCH]  elements 0 .. 53: visits_traj[cell(t, b)]; 54 .. 63: zero.
 *   ring_meta   int8 [capacity][GBL_REPLAY_META_PITCH]    bytes 0 .. 53: mask_traj[cell(t - 1, b)]; byte GBL_REPLAY_META_Z: z_traj[cell(t, b)];
 *                                                         byte GBL_REPLAY_META_MOVER: 1 where mover_traj[cell(t, b)] is non-zero, else 0;
 *                                                         bytes GBL_REPLAY_META_TAG .. + 3: tag, int32 little endian; 60 .. 63: zero.
 *   ring_state  uint64[2] in device memory.  state[0] = the number of rows ever appended: the newest row is in slot
 *     (state[0] - 1) mod capacity and the buffer holds live = min(state[0], capacity) rows.  state[1] = the number of rows the last
 *     append added (its K below).  A fresh buffer is all zeros.  The counters live on the device: append and draw never wait for the
 *     host, the stream alone orders them.
 * The three ring arrays must be 128-byte aligned, ring_state and the workspace 16-byte (GBL_ERR_ALIGN).
 *
 * gbl_replay_append: the valid cells of a window (exactly gbl_training_batch's valid cells, window arguments as there, both layouts),
 * enumerated in ascending (t, b), t outer; K their number, r = 0 .. K - 1 the rank of a cell.  With T0 = state[0] before the call the
 * cell of rank r goes to slot (T0 + r) mod capacity; ranks r < K - capacity are not written at all (a window that alone overflows
 * the ring leaves its last `capacity` rows); afterwards state = (T0 + K, K).  Padding bytes are written as zero -- a ring is
 * comparable byte for byte -- and nothing outside the written slots is touched.  Three launches on the caller's stream, no atomics and
 * no waiting between workgroups: a count (one wavefront per chunk = the 64 boards of one tile at one ply, (plies - 1) * ceil(n / 64)
 * chunks, a ballot each), an exclusive scan of the chunk counts by one workgroup, which also writes the new state, and a scatter (one
 * wavefront per chunk closes its valid rows up and stores them as whole 16-byte vectors).  Ranks are 64-bit.
 *   Workspace.  The caller supplies gbl_replay_workspace_bytes bytes: 32 + 16 per chunk (T0 and K, and per chunk its ballot and the
 *     rank of its first valid cell); that function returns 0 for n outside [1, 2^31] or plies outside [2, 32767] and launches nothing.
 *   Argument errors (GBL_ERR_ARG): plies outside [2, 32767], n outside [1, 2^31], capacity out of range, a missing pointer (all but
 *     obs_traj and ring_obs are required), ring_obs without obs_traj or obs_traj without ring_obs, gbl_collect's stride rules, a
 *     workspace_bytes that is too small.  GBL_ERR_ALIGN: the rules above, and obs_traj / mask_traj / visits_traj 16-byte aligned (whole
 *     tiles are read as 16-byte vectors).
 *
 * gbl_replay_batch: `batch` rows drawn exactly uniformly from the newest rows of the ring, each under a random symmetry.  Sample j:
 *   (w0, w1, w2, w3) = the block Philox4x32-10(ctr = (id_lo, id_hi, 16 call, 7), key = (seed_lo, seed_hi)) with id = sample_base + j --
 *     the generator of gbl_training_batch's attempt 0 on stream 7; there is no attempt loop.  call < 2^26.
 *   live = min(state[0], capacity);  span = recent > 0 ? min(recent, live) : live;  age = (w0 * span) >> 32 -- uniform over the span up
 *     to the multiplication's bias: no age is more likely than another by more than span / 2^32;
 *   slot = (state[0] - 1 - age) mod capacity -- `recent` means the newest `recent` rows --;  s = w2 & sym_mask.
 *   Outputs as gbl_training_batch's (dtypes, shapes, alignment rules; all optional but index_out): the images under s of the row's
 *     observation (needs ring_obs), mask and visits with the row's mover as the agent, z_out = the row's z, index_out[j] = (slot, tag),
 *     sym_out = s.  With live == 0 every sample is gbl_training_batch's failed sample: zero rows, z = GBL_Z_OPEN, index (-1, -1), sym 0.
 *   The draw of sample j depends on (seed, sample_base + j, call), recent and the ring's state alone: not on batch, not on the launch.
 *   Argument errors (GBL_ERR_ARG): capacity out of range, batch < 0 or > 2^31, sym_mask outside [0, 511], call >= 2^26, recent < 0, and
 *     with batch > 0: a missing ring_visits, ring_meta, ring_state or index_out, obs_out without ring_obs.  batch == 0 returns GBL_OK
 *     after the scalar checks.  One launch, one wavefront per 64 samples; allocates nothing, no atomics. */
#define GBL_REPLAY_OBS_PITCH 128   /* bytes per ring_obs row */
#define GBL_REPLAY_VISITS_PITCH 64 /* int16 elements per ring_visits row (128 bytes) */
#define GBL_REPLAY_META_PITCH 64   /* bytes per ring_meta row */
#define GBL_REPLAY_META_Z 54
#define GBL_REPLAY_META_MOVER 55
#define GBL_REPLAY_META_TAG 56
size_t gbl_replay_workspace_bytes(int64_t n, uint32_t plies);
int gbl_replay_append(const int8_t *obs_traj, const int8_t *mask_traj, const int16_t *visits_traj, const int8_t *z_traj,
                      const int8_t *done_traj, const int8_t *mover_traj, int64_t n, uint32_t plies, int64_t ply_stride,
                      int64_t tile_stride, int32_t tag, int8_t *ring_obs, int16_t *ring_visits, int8_t *ring_meta, int64_t capacity,
                      uint64_t *ring_state, void *workspace, size_t workspace_bytes, void *stream);
int gbl_replay_batch(const int8_t *ring_obs, const int16_t *ring_visits, const int8_t *ring_meta, int64_t capacity,
                     const uint64_t *ring_state, int64_t recent, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base,
                     uint32_t call, int8_t *obs_out, int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out,
                     int16_t *sym_out, void *stream);

/* Prioritised replay: a priority per ring row and draws with probability proportional to it.  Nothing above changes: the priorities
 * live in a fourth array, and every function here is exact and bit-defined -- kernels, host flavour and a numpy restatement of this text
 * (tests/replay_prio_restatement.py) agree bit for bit.
 *   ring_prio   int32 [capacity], 128-byte aligned, in slot order.  The weight of a row is w = max(ring_prio[slot], 0): a negative entry
 *     counts as 0.  A fresh buffer is all zeros.
 *   prio_index  a block the caller owns, gbl_replay_prio_index_bytes(capacity) bytes (0 for a capacity out of range), 16-byte aligned,
 *     opaque except for its first two uint64: the ring_state[0] it was built for, and the sum of w over all live rows.
 *
 * gbl_replay_prio_append sets the priorities of the rows that the gbl_replay_append just before it wrote.  PRECONDITION: it follows that
 *   append with the same window arguments (visits_traj, z_traj, done_traj, n, plies, the two strides), the same capacity and ring_state
 *   and the same workspace, untouched since.  With K = state[1] and T0 = state[0] - K the valid cell of rank r gets prio_traj[cell(t, b)]
 *   (int32, indexed as z_traj is: it belongs with visits_traj[cell(t, b)]) or, where prio_traj is NULL, the scalar `value`, at slot
 *   (T0 + r) mod capacity; ranks under the cut (r < K - capacity) are not written, and no other slot is touched.  The device flavour reads
 *   the chunks' ballots, their first ranks, T0 and K from the workspace (one launch, one wavefront per chunk, ranks by mbcnt) and only
 *   checks the window's three arrays for NULL; the host flavour enumerates the cells again and ignores the workspace.
 * gbl_replay_prio_update sets the priorities of drawn rows: for index int32 [batch][2] (the index_out of a draw) and values int32 [batch],
 *   every slot s named by some index[j][0] gets the maximum of values[j] over the j that name it; the old value is replaced, not kept.
 *   Entries whose slot is outside [0, capacity) are skipped (the failed sample's -1 is one).  Two launches on the caller's stream -- the
 *   first stores INT32_MIN to every named slot, the second applies atomicMax -- so the result does not depend on scheduling.  A value
 *   stored negative reads as weight 0.
 * gbl_replay_prio_index builds prio_index from ring_prio and ring_state.  Slots that are not live (slot >= state[0] on a ring that has
 *   not wrapped) count 0 whatever they hold.  Two launches (the prefix sums inside every block of 2 048 slots, a workgroup per block, and
 *   a scan over the blocks by one workgroup), no atomics and no waiting between workgroups.
 * gbl_replay_batch_prio: gbl_replay_batch with a weighted draw.  Sample j:
 *   (w0, w1, w2, w3) = gbl_replay_batch's Philox block on stream 8 (ctr = (id_lo, id_hi, 16 call, 8)); total = state[0], live and span as
 *     there.  The span's rows from oldest to newest are q = 0 .. span - 1 at slot(q) = (total - span + q) mod capacity.
 *   W = sum of w(q);  u = (w0 << 32) | w1;  r = floor(u W / 2^64) (the high half of a 64 x 64 product);
 *   q* = the smallest q with w(0) + .. + w(q) > r;  the sample's slot is slot(q*), its symmetry s = w2 & sym_mask.
 *   A row of weight 0 is never drawn; a row's probability is w / W up to one count in 2^64.
 *   Outputs: every output of gbl_replay_batch as there (index_out = (slot, tag)), prio_out[j] = w(q*) (int32 [batch], optional) and
 *     total_out = (W, span) (uint64 [2], optional, 8-byte aligned, written once per launch).
 *   Every sample is gbl_replay_batch's failed sample (zero rows, z = GBL_Z_OPEN, index (-1, -1), sym 0, prio_out 0) when live == 0, when
 *     W == 0, or when the index's first word is not state[0] (an append happened after the build); then total_out = (0, span).
 *   With an index that is stale only because priorities changed since the build the draw is unspecified, but it still returns a slot
 *     inside [0, capacity) and reads nothing outside the four arrays and the index.
 *   The draw of sample j depends on (seed, sample_base + j, call), recent, the ring's state and the priorities alone.
 *   Sizes: W < 2^62 (any ring of int32 priorities); all sums are uint64.
 *   Argument errors: gbl_replay_batch's, in its order (batch == 0 returns GBL_OK after the scalar checks and writes nothing, total_out
 *     included); then with batch > 0 a missing ring_prio or prio_index (GBL_ERR_ARG).  The other
 *     three: capacity out of range, (batch out of range,) a missing pointer, the window's rules of gbl_replay_append, a workspace_bytes or
 *     index_bytes that is too small (GBL_ERR_ARG).  GBL_ERR_ALIGN: ring_prio 128-byte, ring_state / workspace / prio_index 16-byte,
 *     index / values / prio_traj / prio_out 4-byte, total_out 8-byte.
 *   Measured (one MI355X, profiles/r25/replay_prio.json; a ring of 2^21 slots, batch 65 536): the index build plus the draw
 *     92.5 us against 111.4 us for torch.cumsum + torch.searchsorted + gbl_replay_batch; the draw alone 85.1 us against gbl_replay_batch's
 *     75.4 us; the build alone 11.0 us; gbl_replay_prio_append adds 2.9 us to a 34.5 us append.  NOT MEASURED: whether prioritising
 *     helps a fit. */
size_t gbl_replay_prio_index_bytes(int64_t capacity);
int gbl_replay_prio_append(const int16_t *visits_traj, const int8_t *z_traj, const int8_t *done_traj, const int32_t *prio_traj, int32_t value,
                           int64_t n, uint32_t plies, int64_t ply_stride, int64_t tile_stride, int32_t *ring_prio, int64_t capacity,
                           const uint64_t *ring_state, const void *workspace, size_t workspace_bytes, void *stream);
int gbl_replay_prio_update(const int32_t *index, const int32_t *values, int64_t batch, int32_t *ring_prio, int64_t capacity, void *stream);
int gbl_replay_prio_index(const int32_t *ring_prio, int64_t capacity, const uint64_t *ring_state, void *prio_index, size_t index_bytes,
                          void *stream);
int gbl_replay_batch_prio(const int8_t *ring_obs, const int16_t *ring_visits, const int8_t *ring_meta, int64_t capacity,
                          const uint64_t *ring_state, const int32_t *ring_prio, const void *prio_index, int32_t *prio_out, uint64_t *total_out,
                          int64_t recent, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base, uint32_t call, int8_t *obs_out,
                          int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out, int16_t *sym_out, void *stream);

/* The importance weights of a prioritised draw, bit-defined: prio int32 [batch] is the prio_out of a gbl_replay_batch_prio, weights_out
 * float [batch] what gbl_train_step_weighted takes as row_weight.  The usual weight (W / (span w_j))^beta divided by the batch's largest
 * needs only the batch, W and span cancel:
 *   wmin = the smallest prio[j] > 0 (an integer minimum: any order);
 *   weights_out[j] = prio[j] > 0 ? EXP(-(beta * LOG(float(prio[j]) / float(wmin)))) : 0;   every weight is 0 if no entry is positive.
 * EXP and LOG are gbl_train_step's above, one conversion, one divide, one multiply and one negation around them.  The row at wmin gets
 * exactly 1.0f; the LOG argument lies in [1, 2^31], where LOG is within 0.74746 ulp (measured over 2^20 evenly spaced arguments of
 * [1, 2^31] and the range edges -- 0.60622 ulp -- and over the 2^20 of [1, 54] above, whose maximum it is; asserted as the bound by
 * tests/test_train_weighted.py).  Against float64 (wmin / w)^beta the weights are within 2^-19 relative (measured 1.04e-6).
 * 1 <= batch <= 65 536 and 0 <= beta <= 1 (a NaN beta included: GBL_ERR_ARG), then a missing pointer (GBL_ERR_ARG); prio and weights_out
 * 4-byte aligned (GBL_ERR_ALIGN, device flavour).  One launch, no atomics, no waiting between workgroups: every workgroup finds the
 * minimum over the (L2-resident, at most 256 KB) array itself. */
int gbl_replay_importance(const int32_t *prio, int64_t batch, float beta, float *weights_out, void *stream);

/* Exact tablebase (no counterpart in the reference: the game solved outright, one byte per position).  Integer-only and draws nothing:
 * the kernels, the host flavour and a restatement of this text agree byte for byte.
 *   Inventory.  inventory[3] (int32 on the HOST, read at the call) gives c_k in 0 .. 2, each player's number of pieces of size k.  The
 *     reference's game is (2, 2, 2).  The pieces 2k+1 .. 2k+c_k exist; a smaller inventory is the same rules with fewer pieces.  A state
 *     of an inventory holds only pieces that exist.
 *   Position.  Pieces of equal size are interchangeable and the rules treat the two colours alike (check_for_winner compares the two
 *     colours' lines in the same way), so a position is stored as the side to move sees it: three levels of nine cells, each cell
 *     t = 0 empty, 1 own (the mover's), 2 other; at most c_k own and at most c_k other cells on level k.  A concrete board with
 *     player_2 to move is looked up with the colours swapped.
 *   Index.  code_k = the rank of level k's configuration, in ascending order of sum over pos of t_pos * 3^pos, among the admissible
 *     ones; there are L_k = 1 / 91 / 1 423 of them for c_k = 0 / 1 / 2.  index = (code_2 * L_1 + code_1) * L_0 + code_0, and
 *     positions = L_0 * L_1 * L_2 (2 881 473 967 for (2, 2, 2): an index needs 32 bits, a signed 32-bit number does not hold it).
 *   Moves of the mover.  A piece of size k may go to any cell that holds no piece of level >= k of either colour.  It comes from the
 *     reserve (fewer than c_k own cells on level k) or from an own cell of level k with nothing on a level above it; the source cell
 *     becomes empty.  This is Board.is_legal / play_turn (board.py:82-132) on interchangeable pieces.  After the move
 *     check_for_winner() is read with the reference's last-line-decides rule, as gbl_solve reads it.
 *   Byte.  int8 per position: GBL_TB_TERMINAL where the position already holds a line of either colour (nobody moves from it);
 *     otherwise gbl_solve's V -- +k the mover wins at ply k, -k the mover has lost by ply k, 0 nothing proven (also a mover without a
 *     move).  Here k goes to 126, so "largest rank" is taken with rank(c) = 128 - c for c > 0, 0 for 0, -128 - c for c < 0: the
 *     order of gbl_solve's rank (the shortest win, the unproven, the longest loss) on the wider range.
 *   Sweeps.  Sweep 0 writes GBL_TB_TERMINAL or 0 into every byte of its range.  Sweep k >= 1 looks at every byte of its range that is
 *     still 0 and computes gbl_solve's c(a) for every move a: +1 / -1 where the move decides at once, otherwise from u = the byte of
 *     the position after a as the other side sees it, where u counts as proven only if 1 <= |u| <= k - 1 (so that a sweep in place
 *     does not depend on the order in which positions are visited) and as 0 otherwise.  V = the c(a) of largest rank; the sweep
 *     writes V where |V| == k and nothing elsewhere.
 *   Invariant.  After sweeps 0 .. k over the whole universe every non-terminal byte equals V(position, mover, r = k) of gbl_solve's
 *     text (a non-zero V is the same at every depth that proves it).  A sweep that decides nothing is the fixed point V(., ., infinity).
 *     k stops at 126: a byte never holds +-127, and a caller whose next sweep would be 127 reports an error instead of wrapping.
 *
 * gbl_tb_layout: out[0] = positions, out[1 .. 3] = L_0, L_1, L_2, out[4] = GBL_TB_AUX_BYTES.  Launches nothing; one function for
 *   both flavours.
 * gbl_tb_prepare: fills the caller's `aux` (GBL_TB_AUX_BYTES bytes, the same for every inventory): the rank of each of the 3^9 = 19 683
 *   level configurations for c = 2 (uint16) and c = 1 (uint8), the inverse tables, and the 512 sums of 3^pos over a 9-bit cell set.
 *   The sweep kernel keeps all of it in LDS.
 * gbl_tb_sweep: sweep k over the positions [first, first + count): byte i of the universe is out[i - first].  `table` is the whole
 *   universe (positions bytes) for the look-ups of u; it is not read for k <= 1 and may be NULL there.  out == table + first is the
 *   sweep in place; out and table may alias in any way.  For k >= 1 `out` must hold the range's bytes after sweeps 0 .. k - 1 and
 *   `table` the universe after sweeps 0 .. k - 1 (bytes of sweep k itself may already be there).  The number of non-zero bytes the call
 *   wrote is ADDED to *decided (uint64 in device memory, 8-byte aligned; the caller zeroes it), so that a sweep cut into slices
 *   counts in one place.  0 <= k <= GBL_TB_MAX_SWEEP; count == 0 returns GBL_OK after the scalar checks.
 * gbl_tb_index: index_out int64[n] = the index of board b as to_move[b] sees it, or -1 where the board holds a piece the inventory
 *   lacks or more cells of one colour on a level than c_k.
 * gbl_tb_position: state_out int8[n][27] = position index[b] as a contract state with player_1 to move: own cells positive, on
 *   each level the lowest piece number on the lowest cell.  gbl_tb_index of it with to_move = 0 is index[b].  An index outside
 *   [0, positions) gives a row of 27 bytes GBL_TB_TERMINAL.
 * gbl_tb_probe: gbl_solve's three outputs with r = infinity, read from `table`: for every candidate a -- mask[b] & the legal mask of
 *   to_move[b] (mask NULL: the legal mask), less the actions of pieces the inventory lacks -- c(a) as in a sweep with every non-zero,
 *   non-terminal byte counted as proven.  outcome_out int8[n][54] (GBL_SOLVE_NONE for every other action), value_out int8[n] = the
 *   c(a) of largest rank (0 without a candidate), action_out int32[n] = that candidate, the lowest index on ties (-1 without one);
 *   each may be NULL.  A board gbl_tb_index gives -1 for has no candidate.  On a table that is not complete a 0 reads "not proven by
 *   the sweeps done".  One wavefront per board; state / to_move / mask are read a byte at a time and need no alignment.
 * Argument errors (GBL_ERR_ARG): a missing pointer, an inventory entry outside [0, 2], k outside [0, GBL_TB_MAX_SWEEP], a range that
 *   leaves the universe, table == NULL with k >= 2, n < 0.  GBL_ERR_ALIGN (device flavour): aux 16-byte, decided and the int64 arrays
 *   8-byte, action_out 4-byte aligned.  n == 0 returns GBL_OK after the scalar checks.  Nothing here allocates. */
#define GBL_TB_TERMINAL (-128)
#define GBL_TB_MAX_SWEEP 126
#define GBL_TB_AUX_BYTES 63120
int gbl_tb_layout(const int32_t *inventory, int64_t *out);
int gbl_tb_prepare(const int32_t *inventory, void *aux, void *stream);
int gbl_tb_sweep(const int32_t *inventory, const void *aux, const int8_t *table, int8_t *out, int64_t first, int64_t count, int k,
                 uint64_t *decided, void *stream);
int gbl_tb_index(const int32_t *inventory, const void *aux, const int8_t *state, const int8_t *to_move, int64_t *index_out, int64_t n,
                 void *stream);
int gbl_tb_position(const int32_t *inventory, const void *aux, const int64_t *index, int8_t *state_out, int64_t n, void *stream);
int gbl_tb_probe(const int32_t *inventory, const void *aux, const int8_t *table, const int8_t *state, const int8_t *to_move,
                 const int8_t *mask, int8_t *outcome_out, int8_t *value_out, int32_t *action_out, int64_t n, void *stream);

/* Tablebase targets (no counterpart in the reference): exact training targets for rows in the shape gbl_training_batch and
 * gbl_replay_batch write, or for the replay ring's own rows in place, and a census of the targets they replace.  One launch, no
 * allocation, no atomics; integer-only, so the kernel, the host flavour and a restatement of this text agree byte for byte.
 *   Rows.  n rows; row r of each pitched array lies at base + r * pitch, pitches in ELEMENTS of the array's type: obs int8 (117 per
 *     row), mask int8 (54), visits_in / visits_out int16 (54, one pitch for both), z_in / z_out int8 (1, one pitch for both).  A drawn
 *     batch has the pitches 117 / 54 / 54 / 1; the ring has ring_obs at GBL_REPLAY_OBS_PITCH, ring_meta (the mask) at
 *     GBL_REPLAY_META_PITCH, ring_visits at GBL_REPLAY_VISITS_PITCH and z = ring_meta + GBL_REPLAY_META_Z at GBL_REPLAY_META_PITCH.
 *     Bytes of a pitched row beyond its 117 / 54 / 54 / 1 elements are neither read into the rule nor written.
 *   Skipped rows.  z_in is optional; a row whose z_in byte is GBL_Z_OPEN (the failed sample of both samplers) is skipped: no byte of
 *     its visits_out or z_out row is written.
 *   The rule.  (state, to_move) = gbl_decode_obs of the row's 117 bytes; (outcome[54], value, action) = gbl_tb_probe of that board
 *     with the row's mask bytes as candidates (mask NULL: the legal mask).  A row with action == -1 is UNLABELLED (no candidate, a
 *     board that is no state of the inventory, a mask that removes every move): visits_out = 54 zeros, z_out = GBL_Z_OPEN, so that
 *     gbl_train_step counts it for nothing.  Otherwise, with sign(x) in {-1, 0, +1}: R = the candidates a with
 *     sign(c(a)) == sign(value) (they keep the result), S = those with c(a) == value (the shortest wins, the draws, the longest
 *     losses); O = R for mode GBL_TB_TARGET_RESULT, S for GBL_TB_TARGET_SHORTEST; visits_out[a] = count for a in O and 0 for the other
 *     actions (1 <= count <= 600: a row's sum fits an int16); z_out = sign(value).  visits_out may be NULL.  c(a) is the probe's
 *     outcome BYTE: a table byte of +-127 (no sweep writes one) gives a c(a) of -+128, which reads GBL_SOLVE_NONE there; such a
 *     candidate counts for value and action as in the probe (it ranks like a 0) and belongs to neither set.
 *   Dense outputs (each optional, row r at r * 1 / 54 / 1): value_out int8[n] = value (0 for a skipped or unlabelled row); outcome_out
 *     int8[n][54] = the probe's row (54 times GBL_SOLVE_NONE for a skipped row); census_out int8[n] = -1 for a skipped or unlabelled
 *     row, otherwise bit 0: visits_in is given, the row's 54 old visits are not all <= 0 and their argmax (the lowest index on ties)
 *     lies in R; bit 1: z_in is given and the old z equals the new z; bit 2: the old visits were all <= 0, or visits_in is NULL.
 *   Aliasing.  visits_in == visits_out and z_in == z_out are the in-place forms: a row is read completely before it is written.  Any
 *     other byte an output shares with an input (obs, mask, visits_in, z_in, aux, table) is GBL_ERR_ARG.  Two arrays whose extents
 *     intersect must have the same pitch in bytes (their rows interleave, as z and the mask do in ring_meta); with different
 *     pitches intersecting extents count as an overlap.
 *   Errors, in this order (GBL_ERR_ARG): the inventory, n < 0, mode, count, a pitch smaller than its row (obs; mask if given; visits
 *     if either is given; z); n == 0 returns GBL_OK here; then a missing aux, table, obs or z_out; then the overlaps.
 *     GBL_ERR_ALIGN (device flavour only): aux 16-byte, visits_in / visits_out 2-byte; the byte arrays need no alignment (a batch's
 *     observation rows are 117 bytes apart).
 *   On a table that is not complete a 0 reads "not proven by the sweeps done", as in the probe. */
#define GBL_TB_TARGET_RESULT 0
#define GBL_TB_TARGET_SHORTEST 1
int gbl_tb_targets(const int32_t *inventory, const void *aux, const int8_t *table, const int8_t *obs, int64_t obs_pitch, const int8_t *mask,
                   int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch, const int8_t *z_in, int8_t *z_out,
                   int64_t z_pitch, int mode, int count, int8_t *value_out, int8_t *outcome_out, int8_t *census_out, int64_t n, void *stream);

/* Reanalysis (no counterpart in the reference): fresh search targets for stored rows -- the learned-network counterpart of the tablebase
 * targets above.  The evaluator's search runs again on the position a row's observation holds, and the row's visits become that search's;
 * rows in the shape gbl_training_batch and gbl_replay_batch write, or the replay ring's own rows in place.  One launch, no allocation, no
 * atomics, nothing drawn: the same rows and the same network give the same bytes.  Integer-only, so the kernel, the host flavour and a
 * restatement of this text agree byte for byte.
 *   Rows.  As gbl_tb_targets: n rows, row r of each pitched array at base + r * pitch, pitches in ELEMENTS of the array's type: obs int8
 *     (117 per row), mask int8 (54), visits_in / visits_out int16 (54, one pitch for both), z_in int8 (1).  A drawn batch has the pitches
 *     117 / 54 / 54 / 1; the ring has ring_obs at GBL_REPLAY_OBS_PITCH, ring_meta (the mask) at GBL_REPLAY_META_PITCH, ring_visits at
 *     GBL_REPLAY_VISITS_PITCH and z = ring_meta + GBL_REPLAY_META_Z at GBL_REPLAY_META_PITCH.  Bytes of a pitched row beyond its
 *     117 / 54 / 54 / 1 elements are neither read nor written.
 *   Skipped rows.  z_in is optional; a row whose z_in byte is GBL_Z_OPEN (the failed sample of both samplers) is skipped: no byte of
 *     its visits_out row is written.  z is never written: the value target stays the game's outcome, and an int8 z cannot carry a
 *     fractional root value.
 *   The rule.  (state, to_move) = gbl_decode_obs of the row's 117 bytes; C = the row's mask bytes & the mover's legal mask (mask NULL:
 *     the legal mask).  The search is gbl_tree_search_eval's text unchanged on that board with ev, iterations and explore and the
 *     candidate set C: no root noise, no solver guard.  visits_out[a] = (int16) n_c of the root's child of action a, 0 for the other
 *     actions (iterations <= 512 keeps it inside an int16).  A row with C empty gets 54 zeros, so that gbl_train_step counts it for
 *     nothing.  visits_out may be NULL (the dense outputs alone).
 *   Dense outputs (each optional, row r at r * 1 / 54 / 1 / 1 / 1 / 1): root_value_out int32[n], root_priors_out uint8[n][54],
 *     action_out int32[n] and nodes_out int32[n] are gbl_tree_search_eval's (a row with C empty: the root's q, zeros, -1, 1); a skipped
 *     row holds 0 / zeros / -1 / 0.
 *     drift_out int32[n]: the total variation between the old and the new visit shares, in 1/1024.  With o_a = max(visits_in[a], 0),
 *     So = sum of o_a, n_a = the new visits and Sn = sum of n_a:
 *         drift = (1024 * sum over a of |o_a * Sn - n_a * So|) / (2 * So * Sn)      an unsigned 64-bit division (floor)
 *     and drift = 1024 where So == 0 < Sn.  So <= 54 * 32767 and Sn <= 512, so every term, the sum (at most 2 So Sn < 2^32) and the
 *     divisor fit 32 bits, and the product by 1024 fits 64.  drift = -1 for a skipped row, a row with C empty, or visits_in NULL.
 *     census_out int8[n]: -1 for a skipped row or a row with C empty, otherwise bit 0: visits_in is given, the row's 54 old visits are
 *     not all <= 0 and their argmax (the largest, the lowest index on ties) is the argmax of the new visits row by the same rule;
 *     bit 1: z_in is given, z is -1, 0 or +1 and sign(the root's q) == z; bit 2: the old visits were all <= 0, or visits_in is NULL.
 *   Aliasing.  visits_in == visits_out is the in-place form: a row is read completely before any of it is written.  Any other byte an
 *     output shares with an input (obs, mask, visits_in, z_in, the evaluator's w1 / b1 / w2 / b2) is GBL_ERR_ARG.  Two arrays whose
 *     extents intersect must have the same pitch in bytes (their rows interleave, as z and the mask do in ring_meta); with different
 *     pitches intersecting extents count as an overlap.
 *   Errors, in this order (GBL_ERR_ARG): the evaluator (NULL, hidden, the shifts), iterations (1 .. 512), explore (0 .. 1024), n < 0, a
 *     pitch smaller than its row (obs; mask if given; visits if either is given; z if given); n == 0 returns GBL_OK here; then the
 *     evaluator's four pointers, a missing obs, no output at all; then the overlaps.  GBL_ERR_ALIGN (device flavour only): the
 *     evaluator's arrays 16-byte, visits_in / visits_out 2-byte, root_value_out / action_out / nodes_out / drift_out 4-byte; the byte
 *     arrays need no alignment (a batch's observation rows are 117 bytes apart).
 *   The tree lives in 72 (iterations + 1) bytes of LDS per workgroup, as gbl_tree_search_eval's. */
int gbl_reanalyse(const gbl_evaluator *ev, int iterations, int explore, const int8_t *obs, int64_t obs_pitch, const int8_t *mask,
                  int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch, const int8_t *z_in, int64_t z_pitch,
                  int32_t *root_value_out, uint8_t *root_priors_out, int32_t *action_out, int32_t *nodes_out, int32_t *drift_out,
                  int8_t *census_out, int64_t n, void *stream);

/* Reanalysis with the Gumbel root rule (no counterpart in the reference): gbl_reanalyse with gbl_tree_search_gumbel's search in the place
 * of gbl_tree_search_eval's, so that a stored row's visits become the rule's TARGET ROW -- the completed-Q policy, a byte in 1 .. 255 on
 * every candidate, the kind of row gbl_collect_search_gumbel stores -- from a budget of 8 .. 16 iterations.  One launch, no allocation, no
 * atomics.  Integer-only, so the kernel, the host flavour and a restatement of this text agree byte for byte.
 *   Rows, skipped rows, aliasing.  gbl_reanalyse's text unchanged: the pitches in ELEMENTS, a row whose z_in byte is GBL_Z_OPEN writes no
 *     byte of its visits_out row, visits_in == visits_out is the in-place form, and every other byte an output shares with an input is
 *     GBL_ERR_ARG; gumbel_out is one of the outputs there.
 *   The search.  (state, to_move) = gbl_decode_obs of the row's 117 bytes; C = the row's mask bytes & the mover's legal mask (mask NULL:
 *     the legal mask).  Then gbl_tree_search_gumbel's text unchanged on that board with the candidate set C, with ev, iterations, explore,
 *     considered, gumbel_noise, visit_offset, scale and seed, the board id g = env_base + r (r the row's index in THIS call) and q = call.
 *     With gumbel_noise == 0 nothing is drawn: the same rows and the same network give the same bytes.
 *   visits_out[a] = (int16) target_a, the rule's target byte: 1 .. 255 on C, 0 elsewhere -- what gbl_collect_search_gumbel stores and
 *     gbl_train_step reads unchanged.  A row with C empty gets 54 zeros.  visits_out may be NULL.
 *   Dense outputs (each optional).  root_value_out, root_priors_out and nodes_out are the search's; action_out is the rule's DECISION
 *     (with noise the sampled action); gumbel_out int16[n][54] = g_a (0 outside C, and all 0 without noise; 2-byte aligned).  A row with C
 *     empty holds the root's q, zeros, 1, -1 and a zero Gumbel row; a skipped row 0, zeros, 0, -1 and a zero Gumbel row.
 *     drift_out: gbl_reanalyse's formula with n_a = the new target bytes:
 *         drift = (1024 * sum over a of |o_a * Sn - n_a * So|) / (2 * So * Sn)      an unsigned 64-bit division (floor)
 *     and drift = 1024 where So == 0 (Sn >= 1 on a row with a candidate); -1 for a skipped row, a row with C empty or visits_in NULL.
 *     Now Sn <= 54 * 255 = 13 770 and So <= 54 * 32 767: a single term o_a * Sn or n_a * So still fits 32 bits (at most 451 201 590),
 *     but the sum can reach 2 So Sn, about 4.9e10, and does NOT: the sum and the divisor are unsigned 64-bit, and the product by 1024
 *     (about 5e13) fits 64.  (That is the bytes' own range.  The target rule's bytes of one row sum to at most |C| + 254 <= 308, so a
 *     row this entry point writes keeps the sum below 2^32; the arithmetic does not rest on it.)
 *     census_out: gbl_reanalyse's byte; in bit 0 "the argmax of the new row" is the largest target byte, the lowest index on ties -- not
 *     action_out.
 *   Errors, in this order (GBL_ERR_ARG): the evaluator, iterations and explore as gbl_reanalyse; call >= 2^24; n < 0; env_base + n > 2^42;
 *     considered outside 1 .. 54 (0 is no value here: that search is gbl_reanalyse), gumbel_noise, visit_offset and scale out of range as
 *     gbl_tree_search_gumbel; a pitch smaller than its row; n == 0 returns GBL_OK here; then gbl_reanalyse's pointer and overlap checks
 *     (gumbel_out counts as an output in both).  GBL_ERR_ALIGN (device flavour only): gbl_reanalyse's, then gumbel_out 2-byte.
 *   The tree lives in 72 (iterations + 1) bytes of LDS per workgroup as before: the rule keeps two registers per lane. */
int gbl_reanalyse_gumbel(const gbl_evaluator *ev, int iterations, int explore, int considered, int gumbel_noise, int visit_offset, int scale,
                         uint64_t seed, uint64_t env_base, uint32_t call, const int8_t *obs, int64_t obs_pitch, const int8_t *mask,
                         int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch, const int8_t *z_in,
                         int64_t z_pitch, int32_t *root_value_out, uint8_t *root_priors_out, int32_t *action_out, int32_t *nodes_out,
                         int32_t *drift_out, int8_t *census_out, int16_t *gumbel_out, int64_t n, void *stream);

/* Self-play with the tablebase (no counterpart in the reference): gbl_collect_search_noise with the exact table inside the launch, as a
 * third policy for either side and as a judge of every ply.  The arguments are gbl_collect_search_noise's, then
 *   inventory / aux / table   as gbl_tb_probe takes them (the table complete or not: a 0 reads "not proven by the sweeps done")
 *   tb_mode / tb_count        gbl_tb_targets' mode (the set O) and count, 1 .. 600
 *   tb_outcome_traj int8[cells][54] / tb_value_traj int8[cells] / tb_played_traj int8[cells]   the judge arrays (each may be NULL, none
 *                             needs an alignment)
 * A side's policy is GBL_POLICY_RANDOM, GBL_POLICY_EVAL_TREE or GBL_POLICY_TABLEBASE.  The rule is gbl_collect_search_noise's text with
 * two additions.
 *   The verdict of a ply.  Where a judge array is given or the ply's mover is TABLEBASE: (outcome[54], V, a*) = gbl_tb_probe(inventory,
 *     aux, table, state, to_move, mask = NULL) of the position before the move, as its mover sees it.  tb_outcome_traj[cell] = the outcome
 *     row (54 times GBL_SOLVE_NONE where the board is no state of the inventory or has no candidate); tb_value_traj[cell] = V;
 *     tb_played_traj[cell] = outcome[action] of the action the ply played, GBL_SOLVE_NONE where that action is -1 or no candidate.  The
 *     cell is outcome_traj's: ply t's cell describes ply t's position and mover.
 *   A TABLEBASE mover, a* >= 0.  With R, S and O as gbl_tb_targets defines them from (outcome, V, tb_mode): the visits row holds
 *     tb_count on O and 0 elsewhere; value = sign(V) * 128 * (the row's sum); nodes = 0, root_value = 0, the prior row zeros, the
 *     solver's outcome row GBL_SOLVE_NONE and proven 0.  The action is a* with how = GBL_HOW_TABLE or, while turn[b] < sample_plies,
 *     the visit-proportional draw over that row on stream 4 (gbl_collect_search's rule: k = (r * sum) >> 32, the first action whose
 *     running sum exceeds k, -1 on an empty row) with how = GBL_HOW_TABLE_SAMPLED: uniform over O.  Nothing else is drawn.  A c(a)
 *     of -+128 counts for V and a* and belongs to neither set, as in gbl_tb_targets.
 *   A TABLEBASE mover, a* == -1 (a board outside the inventory, a root without a candidate): exactly a RANDOM side's ply -- the
 *     masked-random draw, how = GBL_HOW_RANDOM, a zero visits row.
 * An EVAL_TREE side keeps its guard, noise, iterations and evaluator; a TABLEBASE side's are not read, as a RANDOM side's.  With no
 * TABLEBASE side and the three judge arrays NULL every array is gbl_collect_search_noise's, bit for bit, and inventory / aux / table may
 * be NULL.  Errors: gbl_collect_search_noise's order, with (GBL_ERR_ARG) a policy outside the three where it reports a policy, then
 * after its depth check tb_mode, tb_count and -- only where a side is TABLEBASE or a judge array is given -- the inventory (NULL, an
 * entry outside 0 .. 2), all before the noise weights; a missing aux, then a missing table, after the three board arrays.  The device
 * flavour asks aux to be 16-byte aligned (GBL_ERR_ALIGN, with the other alignment rules, which are gbl_collect_search_noise's).
 * Nothing about the table's completeness is checked.  Every offset into the table is 64-bit.  gbl_outcome_targets, gbl_training_batch
 * and gbl_replay_append work on these trajectories unchanged.  Allocates nothing. */
#define GBL_POLICY_TABLEBASE 6
#define GBL_HOW_TABLE 6
#define GBL_HOW_TABLE_SAMPLED 7
int gbl_collect_search_tb(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj, int8_t *reward_traj,
                          int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj, int16_t *visits_traj,
                          int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj, int32_t *root_value_traj,
                          uint8_t *priors_traj, int8_t *outcome_traj, int8_t *proven_traj, int64_t n, int64_t ply_stride,
                          int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies,
                          int policy0, int policy1, const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0, int iterations1,
                          int solve_depth0, int solve_depth1, int noise0, int noise1, int explore, int sample_plies, int illegal_mode,
                          int64_t *counters, int32_t *turn, const int32_t *inventory, const void *aux, const int8_t *table, int tb_mode,
                          int tb_count, int8_t *tb_outcome_traj, int8_t *tb_value_traj, int8_t *tb_played_traj, void *stream);

/* Gumbel self-play with the tablebase (no counterpart in the reference): gbl_collect_search_gumbel with the exact table inside the
 * launch, as a third policy for either side and as a judge of every ply.  The arguments are gbl_collect_search_gumbel's up to and
 * including scale, then gbl_collect_search_tb's table block in its order: inventory / aux / table, tb_mode / tb_count, and the judge
 * arrays tb_outcome_traj / tb_value_traj / tb_played_traj (each may be NULL, none needs an alignment).  There is no solver depth, no
 * root noise and no playout cap.  A side's policy is GBL_POLICY_RANDOM, GBL_POLICY_EVAL_TREE or GBL_POLICY_TABLEBASE.  The rule is
 * gbl_collect_search_gumbel's text with gbl_collect_search_tb's two additions, word for word:
 *   The verdict of a ply.  Where a judge array is given or the ply's mover is TABLEBASE: gbl_tb_probe(mask = NULL) of the position
 *     before the move, as its mover sees it; the three judge arrays are written exactly as gbl_collect_search_tb writes them -- the
 *     GBL_SOLVE_NONE rows of a board outside the inventory or without a candidate included, and tb_played = outcome[action] of whatever
 *     the ply played, so a Gumbel ply is judged like any other.
 *   A TABLEBASE mover.  a* >= 0: gbl_collect_search_tb's ply to the byte -- the visits row holds tb_count on O, how = GBL_HOW_TABLE or,
 *     while turn[b] < sample_plies, GBL_HOW_TABLE_SAMPLED with the stream-4 draw; nodes = 0, root_value = 0, the prior row zeros.
 *     a* == -1: a RANDOM side's ply.  Its considered, iterations and evaluator are not read.
 * An EVAL_TREE mover with considered_m > 0 plays gbl_collect_search_gumbel's ply (how = GBL_HOW_GUMBEL, the target row in visits_traj,
 * sample_plies not read); one with considered_m == 0 plays gbl_collect_search_eval's ply, the visit-proportional draw while
 * turn[b] < sample_plies, as in both parents.
 * Two identities hold bit for bit.  With no TABLEBASE side and the three judge arrays NULL every array is gbl_collect_search_gumbel's,
 * and inventory / aux / table may be NULL (tb_mode and tb_count are then not read either).  With both considered 0 every shared array
 * is gbl_collect_search_tb's at depths (0, 0) and noise (0, 0).
 * Errors, all GBL_ERR_ARG, in this order: n < 0; illegal_mode; a policy outside the three; per EVAL_TREE side, player_1 first, its
 * evaluator (NULL, hidden, shifts) and then its iterations / explore; the window (sample_plies < 0, sample_plies > 0 without turn,
 * ply0 + plies > 2^24, env_base + n); then -- only where a side is TABLEBASE or a judge array is given -- tb_mode, tb_count, the
 * inventory (NULL, an entry outside 0 .. 2); a considered outside 0 .. 54 on an EVAL_TREE side; where a side follows the rule,
 * gumbel_noise, visit_offset, scale out of range; n == 0 returns GBL_OK here; state, to_move, done NULL; where the call reads the
 * table a missing aux, then a missing table; plies == 0 returns GBL_OK here; an EVAL_TREE side's weight pointers; the strides.  The
 * device flavour then has its alignment rules (GBL_ERR_ALIGN): gbl_collect_search_gumbel's, among them, after the trajectory's, aux
 * 16-byte aligned where the call reads the table.  A RANDOM or TABLEBASE side's considered, iterations and evaluator are never
 * looked at.  Nothing about the table's completeness is checked.  Every offset into the table is 64-bit.  gbl_outcome_targets,
 * gbl_training_batch and gbl_replay_append work on these trajectories unchanged.  Allocates nothing; the LDS is
 * gbl_collect_search_eval's.  The solver guard is not combined with the table here. */
int gbl_collect_gumbel_tb(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj, int8_t *reward_traj,
                          int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj, int16_t *visits_traj,
                          int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj, int32_t *root_value_traj,
                          uint8_t *priors_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base,
                          uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0,
                          const gbl_evaluator *ev1, int iterations0, int iterations1, int explore, int sample_plies, int illegal_mode,
                          int64_t *counters, int32_t *turn, int considered0, int considered1, int gumbel_noise, int visit_offset,
                          int scale, const int32_t *inventory, const void *aux, const int8_t *table, int tb_mode, int tb_count,
                          int8_t *tb_outcome_traj, int8_t *tb_value_traj, int8_t *tb_played_traj, void *stream);

/* Which kernel a gbl_collect call of this shape runs (no launch; >= 0, or GBL_ERR_ARG): benchmarks and profiles label
 * their records with it instead of re-deriving the library's dispatch rule.
 *   GBL_COLLECT_STREAM  k_collect,  one wavefront per tile of 64 boards, trajectory rows stored non-temporally
 *   GBL_COLLECT_CACHED  k_collect with plain stores (does not exist in the product build: A/B builds only)
 *   GBL_COLLECT_PAIR    k_collect2, two wavefronts per tile (one plays, one stores): grids of up to 2560 tiles
 *   GBL_COLLECT_TRIO    k_collect3, three wavefronts per tile: one plays and hands every ply's position over (one barrier per
 *                       ply), one builds and stores the mask rows, one the observation rows
 *   GBL_COLLECT_GROUP32 k_collect5 (round 6): batches that do not fill the chip and have a mask trajectory -- groups of 32 boards; ONE
 *                       wavefront plays a group (two lanes per board) and leaves every ply's position, legal mask, action and results
 *                       in an LDS ring of 2 x 4 plies; a second wavefront builds the mask rows, stores the scalars and runs the
 *                       sampler's generator, two more the observation rows of 16 boards each; one rendezvous per four plies.
 *                       FULL up to 9 216 boards, MASK_ONLY up to 32 768
 *   GBL_COLLECT_ROLES(la, ko, merge) = 1000 + 100 la + 10 ko + merge:  k_collect_small<la, ko, merge> -- batches that do
 *                       not fill the chip, whose launch lasts as long as ONE wavefront's serial path: role wavefronts that
 *                       share nothing, each playing the whole game and materialising one share of the outputs.  A workgroup
 *                       is a group of 64 / la boards: one scalars wavefront (which also builds the mask rows when merge = 1),
 *                       unless merged one mask wavefront, both with la lanes per board, and ko observation wavefronts of
 *                       la * ko lanes per board over 1 / ko of the group each.  Round 4's small-batch kernel is (4, 1, 0).  Since
 *                       round 6 only launches WITHOUT a mask trajectory (up to 8 192 boards) run it; with one: GBL_COLLECT_GROUP32.
 * (abi_version 2 added GBL_COLLECT_GROUP32; a consumer that switches on the code should treat unknown values as "another kernel".) */
#define GBL_COLLECT_STREAM 0
#define GBL_COLLECT_CACHED 1
#define GBL_COLLECT_PAIR 2
#define GBL_COLLECT_TRIO 4
/* (3 was GBL_COLLECT_SMALL until ABI version 1's role kernel got its forms; the code is retired, not reused: a consumer built
 *  against that header never reads k_collect3 as the small-batch kernel.  The name stays as an alias of the form it stood for.) */
#define GBL_COLLECT_SMALL GBL_COLLECT_ROLES(4, 1, 0) /* deprecated */
#define GBL_COLLECT_GROUP32 5 /* k_collect5 (round 6): groups of 32 boards, one playing wavefront + row wavefronts behind a hand-over ring */
#define GBL_COLLECT_ROLES(la, ko, merge) (1000 + 100 * (la) + 10 * (ko) + (merge))
#define GBL_COLLECT_IS_ROLES(variant) ((variant) >= 1000)
int gbl_collect_variant(int64_t n, uint32_t plies, int with_mask, int with_obs);
/* gbl_collect whose FIRST ply plays caller-supplied actions (first_actions int32[n]; NULL = gbl_collect): the collector
 * step of a policy that lives outside the library against masked-random replies -- the loops of the reference's trainers
 * with a random opponent (gobblet_rl/examples/example_tianshou_DQN.py: MultiAgentPolicyManager([agent, RandomPolicy])) --
 * in ONE launch per decision of the external policy instead of one per ply: with plies = 2, slot 0 receives the given
 * action's ply (illegal or out-of-range actions per illegal_mode, as gbl_step) and slot 1 the sampled reply (ply index
 * ply0 + 1), both with auto-reset; the policy reads slot 1's observation and mask for its next decision.  plies = 1 is
 * gbl_step_into with auto-reset; plies > 2 lets the sampler play on.  Everything else as gbl_collect. */
int gbl_collect_from(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *first_actions, int32_t *actions_traj,
                     int8_t *winner_traj, int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj,
                     int8_t *obs_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed,
                     uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int illegal_mode,
                     int64_t *counters, int32_t *turn, void *stream);
/* gbl_collect_from with the status byte of the caller's actions (first_status int8[n], GBL_STATUS_* as in gbl_step_ex;
 * NULL = gbl_collect_from; needs first_actions). */
int gbl_collect_from_ex(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *first_actions, int8_t *first_status,
                        int32_t *actions_traj, int8_t *winner_traj, int8_t *reward_traj, int8_t *done_traj,
                        int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj, int64_t n, int64_t ply_stride,
                        int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev,
                        uint32_t plies, int illegal_mode, int64_t *counters, int32_t *turn, void *stream);
/* *counter += by, enqueued on the stream (device uint32). */
int gbl_counter_add(uint32_t *counter, uint32_t by, void *stream);

/* Placement helper (no counterpart in the reference: it concerns where the caller puts the two large trajectory
 * arrays of gbl_collect in device memory).  On MI355X two write streams that lie in the same third of the HBM
 * address space (a 96 GiB class -- by its size one of the three die groups of the 12-high stacks) do not overlap:
 * gbl_collect then takes the SUM of what its observation stream and its mask stream take alone (33 us per ply at 2^20
 * boards), against 27 us when the two arrays lie in different classes.  Physical addresses are not
 * visible to a process, so the property is measured: the probe replays gbl_collect's store pattern (64 x 117 bytes
 * into a, 64 x 54 bytes into b per wavefront and slot) with both streams, with a alone and with b alone, and reports
 * the three times in microseconds.  us_both close to us_a + us_b: the two buffers share a class; us_both about 0.8
 * of the sum: they do not.  slot_boards > 0 (a multiple of 128) and plies: the geometry of the time-major trajectory
 * the buffers will hold -- slot t of a at t * slot_boards * 117 bytes, of b at t * slot_boards * 54 -- so that the
 * probe pairs exactly the regions the kernel writes together (it matters when an array straddles two classes);
 * slot_boards = 0: four slots spread over the whole of the smaller buffer.  OVERWRITES both buffers with zeros; blocks
 * the host until the probe has run (not capturable into a graph); buffers of less than about 64 MiB are too small for
 * a meaningful answer. */
int gbl_placement_probe(void *a, int64_t a_bytes, void *b, int64_t b_bytes, int64_t slot_boards, int plies, float *us_both,
                        float *us_a, float *us_b, void *stream);

/* Device memory blocks for the placement search (and for C callers without an allocator of their own): one hipMalloc
 * / hipFree each, on the calling thread's current device, outside any caching allocator -- a block handed back is free
 * for every other user of the device at once, with no process-wide cache flush.  The caller owns a block until it
 * frees it.  gbl_block_alloc returns GBL_ERR_HIP (and leaves *dev_ptr alone) when the device cannot provide the block:
 * the search then stops with what it has.  gbl_device_memory: hipMemGetInfo (either pointer may be NULL); the search
 * caps what it holds by a fraction of the free bytes. */
int gbl_block_alloc(int64_t bytes, void **dev_ptr);
int gbl_block_free(void *dev_ptr);
int gbl_device_memory(int64_t *free_bytes, int64_t *total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GOBBLET_HIP_H */
