// gobblet_env_entries.inc -- the seven entry points of the C ABI that only forward to a longer form with the added arguments at
// their defaults (include/gobblet_hip.h, include/gobblet_cpu.h), written once for both flavours.  gobblet_hip.hip and gobblet_cpu.cpp
// include it inside their extern "C" block with GBL_SYMBOL(fn) the flavour's symbol: gbl_##fn / gbl_cpu_##fn.  A wrapper checks
// nothing: its contract is the longer form's (gobblet_device.h: step_error ... greedy_act_error).

int GBL_SYMBOL(step)(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *actions, int8_t *winner_out, int8_t *reward_out,
                     int8_t *mask_out, int8_t *obs_out, int32_t *turn, int64_t n, int illegal_mode, int auto_reset, void *stream)
{
    return GBL_SYMBOL(step_ex)(state, to_move, done, actions, winner_out, reward_out, mask_out, obs_out, turn, nullptr, nullptr, nullptr,
                               nullptr, nullptr, 0, 0, 0, nullptr, n, illegal_mode, auto_reset, stream);
}

int GBL_SYMBOL(step_into)(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *actions, int8_t *winner_out, int8_t *reward_out,
                          int8_t *mask_out, int8_t *obs_out, int32_t *turn, int32_t *actions_out, int8_t *done_out, int8_t *to_move_out,
                          int64_t n, int illegal_mode, int auto_reset, void *stream)
{
    return GBL_SYMBOL(step_ex)(state, to_move, done, actions, winner_out, reward_out, mask_out, obs_out, turn, actions_out, done_out,
                               to_move_out, nullptr, nullptr, 0, 0, 0, nullptr, n, illegal_mode, auto_reset, stream);
}

int GBL_SYMBOL(sample)(const int8_t *mask, int32_t *actions, int64_t n, uint64_t seed, uint64_t env_base, uint32_t ply, void *stream)
{
    return GBL_SYMBOL(sample_at)(mask, actions, n, seed, env_base, ply, nullptr, stream);
}

int GBL_SYMBOL(rollout)(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_out, int8_t *winner_out, int8_t *reward_out,
                        int8_t *mask_out, int8_t *obs_out, int64_t n, uint64_t seed, uint64_t env_base, uint32_t ply0, uint32_t plies,
                        int illegal_mode, int64_t *counters, int32_t *turn, void *stream)
{
    return GBL_SYMBOL(rollout_at)(state, to_move, done, actions_out, winner_out, reward_out, mask_out, obs_out, n, seed, env_base, ply0,
                                  nullptr, plies, illegal_mode, counters, turn, stream);
}

int GBL_SYMBOL(collect_from)(int8_t *state, int8_t *to_move, int8_t *done, const int32_t *first_actions, int32_t *actions_traj,
                             int8_t *winner_traj, int8_t *reward_traj, int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj,
                             int8_t *obs_traj, int64_t n, int64_t ply_stride, int64_t tile_stride, uint64_t seed, uint64_t env_base,
                             uint32_t ply0, const uint32_t *ply_dev, uint32_t plies, int illegal_mode, int64_t *counters, int32_t *turn,
                             void *stream)
{
    return GBL_SYMBOL(collect_from_ex)(state, to_move, done, first_actions, nullptr, actions_traj, winner_traj, reward_traj, done_traj,
                                       to_move_traj, mask_traj, obs_traj, n, ply_stride, tile_stride, seed, env_base, ply0, ply_dev, plies,
                                       illegal_mode, counters, turn, stream);
}

int GBL_SYMBOL(collect)(int8_t *state, int8_t *to_move, int8_t *done, int32_t *actions_traj, int8_t *winner_traj, int8_t *reward_traj,
                        int8_t *done_traj, int8_t *to_move_traj, int8_t *mask_traj, int8_t *obs_traj, int64_t n, int64_t ply_stride,
                        int64_t tile_stride, uint64_t seed, uint64_t env_base, uint32_t ply0, const uint32_t *ply_dev, uint32_t plies,
                        int illegal_mode, int64_t *counters, int32_t *turn, void *stream)
{
    return GBL_SYMBOL(collect_from)(state, to_move, done, nullptr, actions_traj, winner_traj, reward_traj, done_traj, to_move_traj,
                                    mask_traj, obs_traj, n, ply_stride, tile_stride, seed, env_base, ply0, ply_dev, plies, illegal_mode,
                                    counters, turn, stream);
}

int GBL_SYMBOL(greedy_act)(const int8_t *state, const int8_t *to_move, const int8_t *mask, int8_t *hist, int depth, uint64_t seed,
                           uint64_t env_base, uint32_t call, int32_t *action_out, int32_t *chosen_out, int8_t *cand_mask_out,
                           int8_t *fallback_out, int64_t n, void *stream)
{
    return GBL_SYMBOL(greedy_act_at)(state, to_move, mask, hist, depth, seed, env_base, call, nullptr, action_out, chosen_out, cand_mask_out,
                                     fallback_out, n, stream);
}
