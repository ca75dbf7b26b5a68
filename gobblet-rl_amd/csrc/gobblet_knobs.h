// gobblet_knobs.h -- the ONE place where an experiment build may differ from the product.
//
// The product build (what `_native.build()` / `__graft_entry__.build()` compile and what ships) takes the constants below: its
// kernel source has no A/B switch, no forced dispatch and no build that leaves work out.  An EXPERIMENT build
// (scripts/build_variant.sh: -DGBL_AB_BUILD plus knob macros) includes csrc/gobblet_ab.h instead, which maps the -D macros of
// the measurement scripts (profiles/README.md says which script used which) onto the same names.  A product build with one of
// those macros set is a mistake and does not compile.
#pragma once
#include <stdint.h>

#ifdef GBL_AB_BUILD
#include "gobblet_ab.h"
#else

#if defined(GBL_X_GREEDY_SKIP) || defined(GBL_FORCE_NT) || defined(GBL_FORCE_COLLECT_NT) || defined(GBL_FORCE_COLLECT_PAIR) || \
    defined(GBL_FORCE_COLLECT_SMALL) || defined(GBL_AB_COLLECT_CFG) || defined(GBL_FORCE_GREEDY_SHAPE) ||                     \
    defined(GBL_COLLECT_WAVES_PER_EU) || defined(GBL_CP_WAVES_PER_EU) || defined(GBL_X_GREEDY_PAIR_CAP) || defined(GBL_SOLVE_DEAL) || \
    defined(GBL_IMPORTANCE_ONE_GROUP) || defined(GBL_REANALYSE_GROUPS)
#error "experiment knobs need -DGBL_AB_BUILD (csrc/gobblet_ab.h): the product build has none"
#endif

namespace gbl {
namespace knob {
constexpr int kGreedySkip = 0;            // phases of the greedy decision left out (floor builds: WRONG results, timing only)
constexpr int kGreedyPairCap = 0;         // depth-2 pairs of a block beyond this many dropped (0: none; timing only)
constexpr int kForcedNt = 0;              // store policy of the one-ply kernels pinned (0: by batch size)
constexpr int kForcedCollectNt = -1;      // gbl_collect's trajectory stores: -1 = streamed (the product has no plain-store form)
constexpr int kForcedCollectPair = -1;    // k_collect2 forced on / off (-1: by grid size)
constexpr int kForcedCollectSmall = -1;   // the role kernel's form forced (-1: by batch size)
constexpr int kForcedGreedyShape = 0;     // the greedy kernels' block shape forced (0: by batch size)
inline int collect_cfg_override() { return -1; }  // a form picked at run time (gbl_ab_collect_cfg): none
constexpr int kSolveDeal = 0;             // how k_solve deals its (action, reply) pairs: 0 = interleaved, 1 = off an LDS counter
constexpr int kImportanceOneGroup = 0;    // gbl_replay_importance's launch: 0 = a grid whose workgroups each find the minimum, 1 = one workgroup
constexpr int kReanalyseGroups = 1 << 20; // gbl_reanalyse's grid cap, k_tree_eval's: a workgroup per row up to 2^20 rows (a smaller grid was measured slower), the rest by the stride
}  // namespace knob
}  // namespace gbl

// occupancy pins (see k_collect / k_collect_policy)
#define GBL_KNOB_COLLECT_WAVES_PER_EU 4, 4
#define GBL_KNOB_CP_WAVES_PER_EU 4
// template instantiations only experiment builds carry: more forms of the role kernel (codes appended to SmallForms), more block shapes
// (k_collect with plain stores: kForcedCollectNt >= 0)
#define GBL_KNOB_SMALL_FORMS
#define GBL_KNOB_CP_SHAPES
#define GBL_KNOB_GREEDY_SHAPES
#define GBL_KNOB_EXTRA_ENTRY_POINTS

#endif  // GBL_AB_BUILD

// The Gumbel root rule's table (include/gobblet_hip.h, "Gumbel root search"): GT[k] = round(-ln(-ln((k + 1/2) / 256)) * 16 / ln 2), a
// standard Gumbel variate at the midpoint of the k-th of 256 equal slices of (0, 1), in the logits' unit of 1/16 of an octave.  A
// table of the RULE, not a knob: every build carries the same 256 numbers, and the header prints them.
namespace gbl {
constexpr int16_t kGumbelTable[256] = {
    -42, -38, -35, -34, -32, -31, -30, -29, -28, -28, -27, -26, -26, -25, -24, -24,
    -23, -23, -22, -22, -21, -21, -21, -20, -20, -19, -19, -19, -18, -18, -17, -17,
    -17, -16, -16, -16, -15, -15, -15, -14, -14, -14, -14, -13, -13, -13, -12, -12,
    -12, -11, -11, -11, -11, -10, -10, -10, -10, -9, -9, -9, -8, -8, -8, -8,
    -7, -7, -7, -7, -6, -6, -6, -6, -5, -5, -5, -5, -4, -4, -4, -4,
    -3, -3, -3, -3, -2, -2, -2, -2, -1, -1, -1, -1, 0, 0, 0, 0,
    1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4,
    5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7, 8, 8, 8, 8,
    9, 9, 9, 9, 10, 10, 10, 10, 11, 11, 11, 12, 12, 12, 12, 13,
    13, 13, 13, 14, 14, 14, 15, 15, 15, 15, 16, 16, 16, 17, 17, 17,
    18, 18, 18, 19, 19, 19, 19, 20, 20, 20, 21, 21, 21, 22, 22, 22,
    23, 23, 24, 24, 24, 25, 25, 25, 26, 26, 27, 27, 27, 28, 28, 29,
    29, 29, 30, 30, 31, 31, 32, 32, 33, 33, 33, 34, 34, 35, 35, 36,
    37, 37, 38, 38, 39, 39, 40, 41, 41, 42, 43, 43, 44, 45, 45, 46,
    47, 48, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 59, 60, 61, 63,
    64, 66, 67, 69, 71, 73, 76, 78, 81, 84, 88, 93, 99, 107, 119, 144
};
}  // namespace gbl
