// train_weighted_math.cpp -- TEST INFRASTRUCTURE: train_math.cpp (gobblet_device.h compiled for the host, the library's OWN train_exp and
// train_log behind array-in / array-out wrappers) with the scalar pieces gbl_train_step_weighted and gbl_replay_importance add, so
// that tests/test_train_weighted.py can run them over dense grids.  Built by the test into a temporary directory.
#include "train_math.cpp"

extern "C" {
void train_math_weight(const float *w, float *out, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) out[i] = gbl::train_weight(w[i]);
}
void train_math_priority(const float *lp, const float *lv, float scale, int32_t floor, int32_t cap, int32_t *out, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) out[i] = gbl::train_priority(lp[i], lv[i], scale, floor, cap);
}
void train_math_importance(const int32_t *p, int32_t wmin, float beta, float *out, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) out[i] = gbl::importance_weight(p[i], wmin, beta);
}
}
