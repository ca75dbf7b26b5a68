/* gobblet_cpu.h -- the HOST flavour of the C-ABI of gobblet_hip.h ("each in a device (gbl_*) and host (gbl_cpu_*)
 * flavour with identical signatures"): libgobblet_cpu.so, built from gobblet-rl_amd/csrc/gobblet_cpu.cpp with a plain C++
 * compiler -- no GPU, no HIP runtime.
 *
 * Every compute entry point of gobblet_hip.h exists here under the gbl_cpu_ prefix with the SAME parameter list, argument meaning,
 * error codes and results (bit for bit: the game logic is the device header compiled for the host); see gobblet_hip.h for what
 * each one does and for the reference lines it replaces (gobblet_rl/game/board.py, gobblet.py, greedy_policy.py).  Differences:
 *   - all pointers are HOST pointers; the `stream` argument is ignored (calls are synchronous) and no alignment is asked of buffers;
 *   - the *_at forms read *ply_dev / *call_dev from host memory; `counters` accumulates into its first stripe;
 *   - the device-memory helpers (gbl_pinned_alloc / _free, gbl_block_alloc / _free, gbl_device_memory, gbl_placement_probe,
 *     gbl_collect_variant) have no host flavour; gbl_train_workspace_bytes, gbl_replay_workspace_bytes and gbl_tb_layout are the same functions for
 *     both (they launch nothing);
 *   - the gbl_cpu_tb_* entry points take `aux`, `table` and `decided` in host memory;
 *   - gbl_cpu_replay_append checks its workspace like the device flavour and does not use it; ring_state is host memory;
 *   - gbl_cpu_set_threads(t): boards are dealt over t std::threads (0 = the hardware's; the library reads no environment).
 * The argument checks are the device flavour's own, less its alignment rules: both call the same <name>_error() of
 * gobblet-rl_amd/csrc/gobblet_device.h, and tests/golden/env_arg_errors.json (with the other *_arg_errors.json tables) pins them on both.
 * Threading and devices (gobblet_hip.h has the same paragraph): the library is re-entrant and holds no global state but the one number
 * gbl_cpu_set_threads stores, which is read once per call and changes how many workers a call starts, never a result; any number of
 * host threads may call at the same time, each on buffers of its own.  The error text is per thread: gbl_cpu_last_error() returns what
 * the CALLING thread's last failing call left, "" on a thread that has had none.  There is no device to make current and no stream: a
 * call has finished when it returns.  One object of a caller (boards, a ring and its workspace, a network and its moments) must not be
 * driven from two threads at once.  tests/test_host_threads.py runs two workloads from two threads against the serial run.
 * It is a flavour a caller ASKS for (device="cpu" in the Python layer; BASELINE config 1 "on CPU"), never a fallback of the HIP
 * path, and it is test-independent of oracle/: tests/test_cpu_twin.py compares it with the oracle like the GPU tests do. */
#ifndef GOBBLET_CPU_H
#define GOBBLET_CPU_H
#include "gobblet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int gbl_cpu_set_threads(int threads);
const char *gbl_cpu_last_error(void);
int gbl_cpu_layout_info(int32_t out[6]);
int gbl_cpu_reset(int8_t *state, int8_t *to_move, int8_t *done, int8_t *winner, int64_t n, void *stream);
int gbl_cpu_legal_mask(const int8_t *state, const int8_t *to_move, int8_t *mask, int64_t n, void *stream);
int gbl_cpu_is_legal(const int8_t *state, const int8_t *agent_index, const int32_t *actions, int8_t *out, int64_t n,
                     void *stream);
int gbl_cpu_play_turn(int8_t *state, const int8_t *agent_index, const int32_t *actions, int64_t n, void *stream);
int gbl_cpu_winner(const int8_t *state, int8_t *winner, int64_t n, void *stream);
int gbl_cpu_flatboard(const int8_t *state, int8_t *flat, int64_t n, void *stream);
int gbl_cpu_covered(const int8_t *state, int8_t *cov, int64_t n, void *stream);
int gbl_cpu_validate(const int8_t *state, int8_t *flags, int64_t n, void *stream);
int gbl_cpu_observe(const int8_t *state, const int8_t *to_move, int agent_sel, int8_t *obs, int64_t n, void *stream);
int gbl_cpu_board_eval(int8_t *state, const int8_t *agent_index, const int32_t *actions, int8_t *record_out, int64_t n,
                       void *stream);
int gbl_cpu_step(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *actions, int8_t *winner_out,
                 int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int32_t *turn, int64_t n, int illegal_mode,
                 int auto_reset, void *stream);
int gbl_cpu_step_into(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *actions, int8_t *winner_out,
                      int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int32_t *turn, int32_t *actions_out,
                      int8_t *done_out, int8_t *to_move_out, int64_t n, int illegal_mode, int auto_reset, void *stream);
int gbl_cpu_step_ex(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *actions, int8_t *winner_out,
                    int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int32_t *turn, int32_t *actions_out,
                    int8_t *done_out, int8_t *to_move_out, int8_t *status_out, int32_t *next_actions_out, uint64_t seed,
                    uint64_t env_base, uint32_t ply, const uint32_t *ply_dev, int64_t n, int illegal_mode, int auto_reset,
                    void *stream);
int gbl_cpu_sample(const int8_t *mask, int32_t *actions, int64_t n, uint64_t seed, uint64_t env_base, uint32_t ply,
                   void *stream);
int gbl_cpu_sample_at(const int8_t *mask, int32_t *actions, int64_t n, uint64_t seed, uint64_t env_base, uint32_t ply,
                      const uint32_t *ply_dev, void *stream);
int gbl_cpu_counter_add(uint32_t *counter, uint32_t by, void *stream);
int gbl_cpu_rollout(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_out, int8_t *winner_out,
                    int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int64_t n, uint64_t seed, uint64_t env_base,
                    uint32_t ply0, uint32_t plies, int illegal_mode, int64_t *counters, int32_t *turn, void *stream);
int gbl_cpu_rollout_at(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_out, int8_t *winner_out,
                       int8_t *reward_out, int8_t *mask_out, int8_t *obs_out, int64_t n, uint64_t seed, uint64_t env_base,
                       uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int illegal_mode, int64_t *counters,
                       int32_t *turn, void *stream);
int gbl_cpu_collect(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                    int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                    int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                    const uint32_t *ply_dev, uint32_t plies, int illegal_mode, int64_t *counters, int32_t *turn,
                    void *stream);
int gbl_cpu_collect_from(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *first_actions, int32_t *actions_traj,
                         int8_t *winner_traj, int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj,
                         int8_t *obs_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed,
                         uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int illegal_mode,
                         int64_t *counters, int32_t *turn, void *stream);
int gbl_cpu_collect_from_ex(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *first_actions, int8_t *first_status,
                            int32_t *actions_traj, int8_t *winner_traj, int8_t *reward_traj, int8_t *done_traj,
                            int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj, int64_t n, int64_t ply_stride,
                            int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev,
                            uint32_t plies, int illegal_mode, int64_t *counters, int32_t *turn, void *stream);
int gbl_cpu_collect_policy(int8_t *state, int8_t *to_move, int8_t *done, int8_t *hist, int32_t *actions_traj,
                           int8_t *winner_traj, int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj,
                           int8_t *obs_traj, int32_t *chosen_traj, int8_t *how_traj, int8_t *cand_traj, int64_t n,
                           int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                           const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, int opening_plies,
                           int illegal_mode, int64_t *counters, int32_t *turn, void *stream);
int gbl_cpu_decode_obs(const int8_t *obs, int8_t *state, int8_t *to_move, int64_t n, void *stream);
int gbl_cpu_greedy(const int8_t *state, const int8_t *to_move, const int8_t *mask, const int8_t *hist, int depth,
                   int32_t *action_out, int8_t *cand_mask_out, int8_t *fallback_out, int64_t n, void *stream);
int gbl_cpu_greedy_act(const int8_t *state, const int8_t *to_move, const int8_t *mask, int8_t *hist, int depth,
                       uint64_t seed, uint64_t env_base, uint32_t call, int32_t *action_out, int32_t *chosen_out,
                       int8_t *cand_mask_out, int8_t *fallback_out, int64_t n, void *stream);
int gbl_cpu_greedy_act_at(const int8_t *state, const int8_t *to_move, const int8_t *mask, int8_t *hist, int depth,
                          uint64_t seed, uint64_t env_base, uint32_t call, const uint32_t *call_dev, int32_t *action_out,
                          int32_t *chosen_out, int8_t *cand_mask_out, int8_t *fallback_out, int64_t n, void *stream);
int gbl_cpu_playout_values(const int8_t *state, const int8_t *to_move, const int8_t *mask, int playouts, int max_plies,
                           uint64_t seed, uint64_t env_base, uint32_t call, int32_t *wins_out, int32_t *losses_out,
                           int32_t *action_out, int32_t *plies_out, int64_t n, void *stream);
int gbl_cpu_tree_search(const int8_t *state, const int8_t *to_move, const int8_t *mask, int iterations, int playouts, int max_plies,
                        int explore, uint64_t seed, uint64_t env_base, uint32_t call, int32_t *visits_out, int32_t *wins_out,
                        int32_t *losses_out, int32_t *action_out, int32_t *nodes_out, int32_t *plies_out, int64_t n, void *stream);
int gbl_cpu_solve(const int8_t *state, const int8_t *to_move, const int8_t *mask, int depth, int8_t *outcome_out, int8_t *value_out,
                  int32_t *action_out, int64_t n, void *stream);
int gbl_cpu_evaluate(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, uint8_t *priors_out,
                     int32_t *value_out, int32_t *logits_out, int64_t n, void *stream);
int gbl_cpu_tree_search_eval(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                             int explore, int32_t *visits_out, int32_t *wins_out, int32_t *losses_out, int32_t *action_out,
                             int32_t *nodes_out, int32_t *root_value_out, uint8_t *root_priors_out, int64_t n, void *stream);
int gbl_cpu_tree_search_eval_noise(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                                   int explore, int noise, uint64_t seed, uint64_t env_base, uint32_t call, int32_t *visits_out,
                                   int32_t *wins_out, int32_t *losses_out, int32_t *action_out, int32_t *nodes_out,
                                   int32_t *root_value_out, uint8_t *root_priors_out, uint8_t *root_mixed_out, int64_t n, void *stream);
int gbl_cpu_tree_search_gumbel(const int8_t *state, const int8_t *to_move, const int8_t *mask, const gbl_evaluator *ev, int iterations,
                               int explore, int considered, int gumbel_noise, int visit_offset, int scale, uint64_t seed,
                               uint64_t env_base, uint32_t call, int32_t *visits_out, int32_t *wins_out, int32_t *losses_out,
                               int32_t *action_out, int32_t *nodes_out, int32_t *root_value_out, uint8_t *root_priors_out,
                               uint8_t *target_out, int16_t *gumbel_out, int64_t n, void *stream);
int gbl_cpu_collect_search(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                           int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                           int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                           int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                           const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, int iterations0, int iterations1,
                           int playouts0, int playouts1, int max_plies, int explore, int sample_plies, int illegal_mode,
                           int64_t *counters, int32_t *turn, void *stream);
int gbl_cpu_collect_search_eval(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                                int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                                int32_t *root_value_traj, uint8_t *priors_traj, int64_t n, int64_t ply_stride, int64_t tile_stride,
                                uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int policy0,
                                int policy1, const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0, int iterations1,
                                int explore, int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn, void *stream);
int gbl_cpu_collect_search_solve(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                 int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                                 int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                                 int32_t *root_value_traj, uint8_t *priors_traj, int8_t *outcome_traj, int8_t *proven_traj, int64_t n,
                                 int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                                 const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0,
                                 const gbl_evaluator *ev1, int iterations0, int iterations1, int solve_depth0, int solve_depth1, int explore,
                                 int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn, void *stream);
int gbl_cpu_collect_search_noise(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                 int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                                 int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                                 int32_t *root_value_traj, uint8_t *priors_traj, int8_t *outcome_traj, int8_t *proven_traj, int64_t n,
                                 int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                                 const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0,
                                 const gbl_evaluator *ev1, int iterations0, int iterations1, int solve_depth0, int solve_depth1, int noise0,
                                 int noise1, int explore, int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn,
                                 void *stream);
int gbl_cpu_collect_search_cap(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                               int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                               int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                               int32_t *root_value_traj, uint8_t *priors_traj, int8_t *outcome_traj, int8_t *proven_traj, int64_t n,
                               int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                               const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0,
                               const gbl_evaluator *ev1, int iterations0, int iterations1, int solve_depth0, int solve_depth1, int noise0,
                               int noise1, int explore, int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn,
                               int fast_iterations0, int fast_iterations1, int full_share0, int full_share1, void *stream);
int gbl_cpu_collect_search_gumbel(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                  int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                                  int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                                  int32_t *root_value_traj, uint8_t *priors_traj, int64_t n, int64_t ply_stride, int64_t tile_stride,
                                  uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int policy0,
                                  int policy1, const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0, int iterations1,
                                  int explore, int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn, int considered0,
                                  int considered1, int gumbel_noise, int visit_offset, int scale, void *stream);
int gbl_cpu_collect_gumbel_solve(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                 int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                                 int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                                 int32_t *root_value_traj, uint8_t *priors_traj, int8_t *outcome_traj, int8_t *proven_traj, int64_t n,
                                 int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                                 const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0,
                                 const gbl_evaluator *ev1, int iterations0, int iterations1, int solve_depth0, int solve_depth1, int explore,
                                 int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn, int considered0, int considered1,
                                 int gumbel_noise, int visit_offset, int scale, void *stream);
int gbl_cpu_collect_search_tb(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj, int8_t *reward_traj,
                              int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj, int16_t *visits_traj,
                              int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj, int32_t *root_value_traj,
                              uint8_t *priors_traj, int8_t *outcome_traj, int8_t *proven_traj, int64_t n, int64_t ply_stride,
                              int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies,
                              int policy0, int policy1, const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0, int iterations1,
                              int solve_depth0, int solve_depth1, int noise0, int noise1, int explore, int sample_plies, int illegal_mode,
                              int64_t *counters, int32_t *turn, const int32_t *inventory, const void *aux, const int8_t *table, int tb_mode,
                              int tb_count, int8_t *tb_outcome_traj, int8_t *tb_value_traj, int8_t *tb_played_traj, void *stream);
int gbl_cpu_collect_gumbel_tb(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj, int8_t *reward_traj,
                              int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj, int16_t *visits_traj,
                              int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj, int32_t *root_value_traj,
                              uint8_t *priors_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base,
                              uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0,
                              const gbl_evaluator *ev1, int iterations0, int iterations1, int explore, int sample_plies, int illegal_mode,
                              int64_t *counters, int32_t *turn, int considered0, int considered1, int gumbel_noise, int visit_offset,
                              int scale, const int32_t *inventory, const void *aux, const int8_t *table, int tb_mode, int tb_count,
                              int8_t *tb_outcome_traj, int8_t *tb_value_traj, int8_t *tb_played_traj, void *stream);
int gbl_cpu_outcome_targets(const int8_t *done_traj, const int8_t *reward_traj, const int8_t *mover_traj, int8_t *z_traj,
                            int16_t *plies_left_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint32_t plies,
                            void *stream);
int gbl_cpu_symmetry_apply(const int16_t *sym, int sym_all, const int8_t *agent, const int8_t *state_in, int8_t *state_out,
                           const int8_t *obs_in, int8_t *obs_out, const int8_t *mask_in, int8_t *mask_out, const int16_t *visits_in,
                           int16_t *visits_out, const uint8_t *priors_in, uint8_t *priors_out, const int32_t *actions_in,
                           int32_t *actions_out, int64_t n, void *stream);
int gbl_cpu_training_batch(const int8_t *obs_traj, const int8_t *mask_traj, const int16_t *visits_traj, const int8_t *z_traj,
                           const int8_t *done_traj, const int8_t *mover_traj, int64_t n, uint32_t plies, int64_t ply_stride,
                           int64_t tile_stride, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base, uint32_t call,
                           int8_t *obs_out, int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out, int16_t *sym_out,
                           void *stream);
int gbl_cpu_train_step(const int8_t *obs, const int8_t *mask, const int16_t *visits, const int8_t *z, int64_t batch, int hidden,
                       float *params, float *adam_m, float *adam_v, const gbl_train_hyper *hyper, float *grad_out, float *stats_out,
                       void *workspace, int64_t workspace_bytes, void *stream);
int gbl_cpu_train_step_weighted(const int8_t *obs, const int8_t *mask, const int16_t *visits, const int8_t *z, int64_t batch, int hidden,
                                float *params, float *adam_m, float *adam_v, const gbl_train_hyper *hyper, const float *row_weight,
                                float *row_loss_out, int32_t *prio_out, float prio_scale, int32_t prio_floor, int32_t prio_cap, float *grad_out,
                                float *stats_out, void *workspace, int64_t workspace_bytes, void *stream);
int gbl_cpu_replay_importance(const int32_t *prio, int64_t batch, float beta, float *weights_out, void *stream);
int gbl_cpu_replay_append(const int8_t *obs_traj, const int8_t *mask_traj, const int16_t *visits_traj, const int8_t *z_traj,
                          const int8_t *done_traj, const int8_t *mover_traj, int64_t n, uint32_t plies, int64_t ply_stride,
                          int64_t tile_stride, int32_t tag, int8_t *ring_obs, int16_t *ring_visits, int8_t *ring_meta, int64_t capacity,
                          uint64_t *ring_state, void *workspace, size_t workspace_bytes, void *stream);
int gbl_cpu_replay_batch(const int8_t *ring_obs, const int16_t *ring_visits, const int8_t *ring_meta, int64_t capacity,
                         const uint64_t *ring_state, int64_t recent, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base,
                         uint32_t call, int8_t *obs_out, int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out,
                         int16_t *sym_out, void *stream);
/* (gbl_replay_prio_index_bytes is one function for both flavours; gbl_cpu_replay_prio_append enumerates the window's cells again and
 * does not use the workspace) */
int gbl_cpu_replay_prio_append(const int16_t *visits_traj, const int8_t *z_traj, const int8_t *done_traj, const int32_t *prio_traj, int32_t value,
                               int64_t n, uint32_t plies, int64_t ply_stride, int64_t tile_stride, int32_t *ring_prio, int64_t capacity,
                               const uint64_t *ring_state, const void *workspace, size_t workspace_bytes, void *stream);
int gbl_cpu_replay_prio_update(const int32_t *index, const int32_t *values, int64_t batch, int32_t *ring_prio, int64_t capacity, void *stream);
int gbl_cpu_replay_prio_index(const int32_t *ring_prio, int64_t capacity, const uint64_t *ring_state, void *prio_index, size_t index_bytes,
                              void *stream);
int gbl_cpu_replay_batch_prio(const int8_t *ring_obs, const int16_t *ring_visits, const int8_t *ring_meta, int64_t capacity,
                              const uint64_t *ring_state, const int32_t *ring_prio, const void *prio_index, int32_t *prio_out,
                              uint64_t *total_out, int64_t recent, int64_t batch, int sym_mask, uint64_t seed, uint64_t sample_base,
                              uint32_t call, int8_t *obs_out, int8_t *mask_out, int16_t *visits_out, int8_t *z_out, int32_t *index_out,
                              int16_t *sym_out, void *stream);
int gbl_cpu_tb_prepare(const int32_t *inventory, void *aux, void *stream);
int gbl_cpu_tb_sweep(const int32_t *inventory, const void *aux, const int8_t *table, int8_t *out, int64_t first, int64_t count, int k,
                     uint64_t *decided, void *stream);
int gbl_cpu_tb_index(const int32_t *inventory, const void *aux, const int8_t *state, const int8_t *to_move, int64_t *index_out, int64_t n,
                     void *stream);
int gbl_cpu_tb_position(const int32_t *inventory, const void *aux, const int64_t *index, int8_t *state_out, int64_t n, void *stream);
int gbl_cpu_tb_probe(const int32_t *inventory, const void *aux, const int8_t *table, const int8_t *state, const int8_t *to_move,
                     const int8_t *mask, int8_t *outcome_out, int8_t *value_out, int32_t *action_out, int64_t n, void *stream);
int gbl_cpu_tb_targets(const int32_t *inventory, const void *aux, const int8_t *table, const int8_t *obs, int64_t obs_pitch, const int8_t *mask,
                       int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch, const int8_t *z_in,
                       int8_t *z_out, int64_t z_pitch, int mode, int count, int8_t *value_out, int8_t *outcome_out, int8_t *census_out,
                       int64_t n, void *stream);
int gbl_cpu_reanalyse(const gbl_evaluator *ev, int iterations, int explore, const int8_t *obs, int64_t obs_pitch, const int8_t *mask,
                      int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch, const int8_t *z_in,
                      int64_t z_pitch, int32_t *root_value_out, uint8_t *root_priors_out, int32_t *action_out, int32_t *nodes_out,
                      int32_t *drift_out, int8_t *census_out, int64_t n, void *stream);
int gbl_cpu_reanalyse_gumbel(const gbl_evaluator *ev, int iterations, int explore, int considered, int gumbel_noise, int visit_offset,
                             int scale, uint64_t seed, uint64_t env_base, uint32_t call, const int8_t *obs, int64_t obs_pitch,
                             const int8_t *mask, int64_t mask_pitch, const int16_t *visits_in, int16_t *visits_out, int64_t visits_pitch,
                             const int8_t *z_in, int64_t z_pitch, int32_t *root_value_out, uint8_t *root_priors_out, int32_t *action_out,
                             int32_t *nodes_out, int32_t *drift_out, int8_t *census_out, int16_t *gumbel_out, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
