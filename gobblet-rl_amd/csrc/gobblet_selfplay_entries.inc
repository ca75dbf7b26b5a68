// gobblet_selfplay_entries.inc -- the nine self-play entry points of the C ABI (gbl_collect_search and its _eval, _solve, _noise,
// _cap, _gumbel and _tb, gbl_collect_gumbel_solve and gbl_collect_gumbel_tb; include/gobblet_hip.h, include/gobblet_cpu.h), written once for both flavours.  gobblet_hip.hip and
// gobblet_cpu.cpp include it inside their extern "C" block, after their runner, with
//   GBL_SYMBOL(fn)              the flavour's symbol: gbl_##fn / gbl_cpu_##fn
//   GBL_SELFPLAY_RUN(name, call, stream)  the flavour's runner on a filled SelfplayCall<gbl_evaluator>, under the entry point's name
// A wrapper fills what every member has through selfplay_common and then names, field by field, what its member adds; whatever it does
// not name stays 0 / NULL (gobblet_device.h: SelfplayCall).

// What every member has: the boards, the trajectory arrays (t: as many of the 19 as the member has, in SelfplayTraj's order; the rest
// NULL), the window, the policies, the budgets and the shared tail.
static inline SelfplayCall<gbl_evaluator> selfplay_common(SelfplayRun run, int8_t *state, int8_t *to_move, int8_t *done, const SelfplayTraj &t,
                                                          int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed,
                                                          uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies,
                                                          int policy0, int policy1, int iterations0, int iterations1, int explore,
                                                          int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn)
{
    SelfplayCall<gbl_evaluator> c{};
    c.run = run;
    c.state = state, c.to_move = to_move, c.done = done;
    c.traj = t;
    c.n = n, c.ply_stride = ply_stride, c.tile_stride = tile_stride;
    c.seed = seed, c.env_base = env_base;
    c.ply0 = ply0, c.ply_dev = ply_dev, c.plies = plies;
    c.policy[0] = policy0, c.policy[1] = policy1;
    c.iterations[0] = iterations0, c.iterations[1] = iterations1;
    c.explore = explore, c.sample_plies = sample_plies, c.illegal_mode = illegal_mode;
    c.counters = counters, c.turn = turn;
    return c;
}

int GBL_SYMBOL(collect_search)(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                        int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                                        int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj, int8_t *mover_traj,
                                        int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                                        const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, int iterations0, int iterations1,
                                        int playouts0, int playouts1, int max_plies, int explore, int sample_plies, int illegal_mode,
                                        int64_t *counters, int32_t *turn, void *stream)
{
    SelfplayCall<gbl_evaluator> c = selfplay_common(
        kRunSearch, state, to_move, done,
        {actions_traj, winner_traj, reward_traj, done_traj, to_move_traj, mask_traj, obs_traj, visits_traj, value_traj, nodes_traj, how_traj,
         mover_traj},
        n, ply_stride, tile_stride, seed, env_base, ply0, ply_dev, plies, policy0, policy1, iterations0, iterations1, explore, sample_plies,
        illegal_mode, counters, turn);
    c.playouts[0] = playouts0, c.playouts[1] = playouts1;
    c.max_plies = max_plies;
    return GBL_SELFPLAY_RUN("gbl_collect_search", c, stream);
}

int GBL_SYMBOL(collect_search_eval)(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                             int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj,
                                             int8_t *obs_traj, int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj,
                                             int8_t *how_traj, int8_t *mover_traj, int32_t *root_value_traj, uint8_t *priors_traj, int64_t n,
                                             int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0,
                                             const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0,
                                             const gbl_evaluator *ev1, int iterations0, int iterations1, int explore, int sample_plies,
                                             int illegal_mode, int64_t *counters, int32_t *turn, void *stream)
{
    SelfplayCall<gbl_evaluator> c = selfplay_common(
        kRunEval, state, to_move, done,
        {actions_traj, winner_traj, reward_traj, done_traj, to_move_traj, mask_traj, obs_traj, visits_traj, value_traj, nodes_traj, how_traj,
         mover_traj, root_value_traj, priors_traj},
        n, ply_stride, tile_stride, seed, env_base, ply0, ply_dev, plies, policy0, policy1, iterations0, iterations1, explore, sample_plies,
        illegal_mode, counters, turn);
    c.ev[0] = ev0, c.ev[1] = ev1;
    return GBL_SELFPLAY_RUN("gbl_collect_search_eval", c, stream);
}

int GBL_SYMBOL(collect_search_gumbel)(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                               int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj,
                                               int8_t *obs_traj, int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj,
                                               int8_t *how_traj, int8_t *mover_traj, int32_t *root_value_traj, uint8_t *priors_traj,
                                               int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base,
                                               uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1,
                                               const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0, int iterations1,
                                               int explore, int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn,
                                               int considered0, int considered1, int gumbel_noise, int visit_offset, int scale, void *stream)
{
    SelfplayCall<gbl_evaluator> c = selfplay_common(
        kRunEval, state, to_move, done,
        {actions_traj, winner_traj, reward_traj, done_traj, to_move_traj, mask_traj, obs_traj, visits_traj, value_traj, nodes_traj, how_traj,
         mover_traj, root_value_traj, priors_traj},
        n, ply_stride, tile_stride, seed, env_base, ply0, ply_dev, plies, policy0, policy1, iterations0, iterations1, explore, sample_plies,
        illegal_mode, counters, turn);
    c.ev[0] = ev0, c.ev[1] = ev1;
    c.gumbel = 1;
    c.considered[0] = considered0, c.considered[1] = considered1;
    c.gumbel_noise = gumbel_noise, c.visit_offset = visit_offset, c.scale = scale;
    return GBL_SELFPLAY_RUN("gbl_collect_search_gumbel", c, stream);
}

int GBL_SYMBOL(collect_search_solve)(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                              int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj,
                                              int8_t *obs_traj, int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj,
                                              int8_t *how_traj, int8_t *mover_traj, int32_t *root_value_traj, uint8_t *priors_traj,
                                              int8_t *outcome_traj, int8_t *proven_traj, int64_t n, int64_t ply_stride, int64_t tile_stride,
                                              uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies,
                                              int policy0, int policy1, const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0,
                                              int iterations1, int solve_depth0, int solve_depth1, int explore, int sample_plies,
                                              int illegal_mode, int64_t *counters, int32_t *turn, void *stream)
{
    SelfplayCall<gbl_evaluator> c = selfplay_common(
        kRunSolve, state, to_move, done,
        {actions_traj, winner_traj, reward_traj, done_traj, to_move_traj, mask_traj, obs_traj, visits_traj, value_traj, nodes_traj, how_traj,
         mover_traj, root_value_traj, priors_traj, outcome_traj, proven_traj},
        n, ply_stride, tile_stride, seed, env_base, ply0, ply_dev, plies, policy0, policy1, iterations0, iterations1, explore, sample_plies,
        illegal_mode, counters, turn);
    c.ev[0] = ev0, c.ev[1] = ev1;
    c.solve_depth[0] = solve_depth0, c.solve_depth[1] = solve_depth1;
    return GBL_SELFPLAY_RUN("gbl_collect_search_solve", c, stream);
}

int GBL_SYMBOL(collect_gumbel_solve)(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                              int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj,
                                              int8_t *obs_traj, int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj,
                                              int8_t *how_traj, int8_t *mover_traj, int32_t *root_value_traj, uint8_t *priors_traj,
                                              int8_t *outcome_traj, int8_t *proven_traj, int64_t n, int64_t ply_stride, int64_t tile_stride,
                                              uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies,
                                              int policy0, int policy1, const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0,
                                              int iterations1, int solve_depth0, int solve_depth1, int explore, int sample_plies,
                                              int illegal_mode, int64_t *counters, int32_t *turn, int considered0, int considered1,
                                              int gumbel_noise, int visit_offset, int scale, void *stream)
{
    SelfplayCall<gbl_evaluator> c = selfplay_common(
        kRunSolve, state, to_move, done,
        {actions_traj, winner_traj, reward_traj, done_traj, to_move_traj, mask_traj, obs_traj, visits_traj, value_traj, nodes_traj, how_traj,
         mover_traj, root_value_traj, priors_traj, outcome_traj, proven_traj},
        n, ply_stride, tile_stride, seed, env_base, ply0, ply_dev, plies, policy0, policy1, iterations0, iterations1, explore, sample_plies,
        illegal_mode, counters, turn);
    c.ev[0] = ev0, c.ev[1] = ev1;
    c.solve_depth[0] = solve_depth0, c.solve_depth[1] = solve_depth1;
    c.gumbel = 1;
    c.considered[0] = considered0, c.considered[1] = considered1;
    c.gumbel_noise = gumbel_noise, c.visit_offset = visit_offset, c.scale = scale;
    return GBL_SELFPLAY_RUN("gbl_collect_gumbel_solve", c, stream);
}

int GBL_SYMBOL(collect_search_noise)(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                              int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj,
                                              int8_t *obs_traj, int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj,
                                              int8_t *how_traj, int8_t *mover_traj, int32_t *root_value_traj, uint8_t *priors_traj,
                                              int8_t *outcome_traj, int8_t *proven_traj, int64_t n, int64_t ply_stride, int64_t tile_stride,
                                              uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies,
                                              int policy0, int policy1, const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0,
                                              int iterations1, int solve_depth0, int solve_depth1, int noise0, int noise1, int explore,
                                              int sample_plies, int illegal_mode, int64_t *counters, int32_t *turn, void *stream)
{
    SelfplayCall<gbl_evaluator> c = selfplay_common(
        kRunSolve, state, to_move, done,
        {actions_traj, winner_traj, reward_traj, done_traj, to_move_traj, mask_traj, obs_traj, visits_traj, value_traj, nodes_traj, how_traj,
         mover_traj, root_value_traj, priors_traj, outcome_traj, proven_traj},
        n, ply_stride, tile_stride, seed, env_base, ply0, ply_dev, plies, policy0, policy1, iterations0, iterations1, explore, sample_plies,
        illegal_mode, counters, turn);
    c.ev[0] = ev0, c.ev[1] = ev1;
    c.solve_depth[0] = solve_depth0, c.solve_depth[1] = solve_depth1;
    c.noise[0] = noise0, c.noise[1] = noise1;
    return GBL_SELFPLAY_RUN("gbl_collect_search_noise", c, stream);
}

int GBL_SYMBOL(collect_search_cap)(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                            int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                                            int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj,
                                            int8_t *mover_traj, int32_t *root_value_traj, uint8_t *priors_traj, int8_t *outcome_traj,
                                            int8_t *proven_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed,
                                            uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int policy0,
                                            int policy1, const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0, int iterations1,
                                            int solve_depth0, int solve_depth1, int noise0, int noise1, int explore, int sample_plies,
                                            int illegal_mode, int64_t *counters, int32_t *turn, int fast_iterations0, int fast_iterations1,
                                            int full_share0, int full_share1, void *stream)
{
    SelfplayCall<gbl_evaluator> c = selfplay_common(
        kRunSolve, state, to_move, done,
        {actions_traj, winner_traj, reward_traj, done_traj, to_move_traj, mask_traj, obs_traj, visits_traj, value_traj, nodes_traj, how_traj,
         mover_traj, root_value_traj, priors_traj, outcome_traj, proven_traj},
        n, ply_stride, tile_stride, seed, env_base, ply0, ply_dev, plies, policy0, policy1, iterations0, iterations1, explore, sample_plies,
        illegal_mode, counters, turn);
    c.ev[0] = ev0, c.ev[1] = ev1;
    c.solve_depth[0] = solve_depth0, c.solve_depth[1] = solve_depth1;
    c.noise[0] = noise0, c.noise[1] = noise1;
    c.cap = 1;
    c.fast[0] = fast_iterations0, c.fast[1] = fast_iterations1;
    c.share[0] = full_share0, c.share[1] = full_share1;
    return GBL_SELFPLAY_RUN("gbl_collect_search_cap", c, stream);
}

int GBL_SYMBOL(collect_search_tb)(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                           int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                                           int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj,
                                           int8_t *mover_traj, int32_t *root_value_traj, uint8_t *priors_traj, int8_t *outcome_traj,
                                           int8_t *proven_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed,
                                           uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int policy0, int policy1,
                                           const gbl_evaluator *ev0, const gbl_evaluator *ev1, int iterations0, int iterations1,
                                           int solve_depth0, int solve_depth1, int noise0, int noise1, int explore, int sample_plies,
                                           int illegal_mode, int64_t *counters, int32_t *turn, const int32_t *inventory, const void *aux,
                                           const int8_t *table, int tb_mode, int tb_count, int8_t *tb_outcome_traj, int8_t *tb_value_traj,
                                           int8_t *tb_played_traj, void *stream)
{
    SelfplayCall<gbl_evaluator> c = selfplay_common(
        kRunTb, state, to_move, done,
        {actions_traj, winner_traj, reward_traj, done_traj, to_move_traj, mask_traj, obs_traj, visits_traj, value_traj, nodes_traj, how_traj,
         mover_traj, root_value_traj, priors_traj, outcome_traj, proven_traj, tb_outcome_traj, tb_value_traj, tb_played_traj},
        n, ply_stride, tile_stride, seed, env_base, ply0, ply_dev, plies, policy0, policy1, iterations0, iterations1, explore, sample_plies,
        illegal_mode, counters, turn);
    c.ev[0] = ev0, c.ev[1] = ev1;
    c.solve_depth[0] = solve_depth0, c.solve_depth[1] = solve_depth1;
    c.noise[0] = noise0, c.noise[1] = noise1;
    c.inventory = inventory, c.aux = aux, c.table = table;
    c.tb_mode = tb_mode, c.tb_count = tb_count;
    return GBL_SELFPLAY_RUN("gbl_collect_search_tb", c, stream);
}

int GBL_SYMBOL(collect_gumbel_tb)(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj,
                                           int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj,
                                           int16_t *visits_traj, int32_t *value_traj, int32_t *nodes_traj, int8_t *how_traj,
                                           int8_t *mover_traj, int32_t *root_value_traj, uint8_t *priors_traj, int64_t n, int64_t ply_stride,
                                           int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev,
                                           uint32_t plies, int policy0, int policy1, const gbl_evaluator *ev0, const gbl_evaluator *ev1,
                                           int iterations0, int iterations1, int explore, int sample_plies, int illegal_mode,
                                           int64_t *counters, int32_t *turn, int considered0, int considered1, int gumbel_noise,
                                           int visit_offset, int scale, const int32_t *inventory, const void *aux, const int8_t *table,
                                           int tb_mode, int tb_count, int8_t *tb_outcome_traj, int8_t *tb_value_traj, int8_t *tb_played_traj,
                                           void *stream)
{
    SelfplayCall<gbl_evaluator> c = selfplay_common(
        kRunTb, state, to_move, done,
        {actions_traj, winner_traj, reward_traj, done_traj, to_move_traj, mask_traj, obs_traj, visits_traj, value_traj, nodes_traj, how_traj,
         mover_traj, root_value_traj, priors_traj, nullptr, nullptr, tb_outcome_traj, tb_value_traj, tb_played_traj},
        n, ply_stride, tile_stride, seed, env_base, ply0, ply_dev, plies, policy0, policy1, iterations0, iterations1, explore, sample_plies,
        illegal_mode, counters, turn);
    c.ev[0] = ev0, c.ev[1] = ev1;
    c.gumbel = 1;
    c.considered[0] = considered0, c.considered[1] = considered1;
    c.gumbel_noise = gumbel_noise, c.visit_offset = visit_offset, c.scale = scale;
    c.inventory = inventory, c.aux = aux, c.table = table;
    c.tb_mode = tb_mode, c.tb_count = tb_count;
    return GBL_SELFPLAY_RUN("gbl_collect_gumbel_tb", c, stream);
}
