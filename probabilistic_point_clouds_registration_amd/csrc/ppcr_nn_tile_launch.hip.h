// Host-side handshake between the C-ABI translation unit (ppcr_hip.hip) and the K1 translation units
// (ppcr_nn_tile.hip, compiled once per list width M): everything one K1 launch needs, by value.
#pragma once
#include "ppcr_device.hip.h"
#include "ppcr_k1_plan.hpp"

namespace ppcr {

struct TileLaunch {
    K1Plan plan;                  // which kernels run, on what grids (plan_k1: the caller sizes its buffers from the same plan)
    hipStream_t stream;
    float4 *src;                  // the (sorted) source; moved in place when pm.enabled
    int ns;
    const float4 *tgt;            // the cell-sorted target
    const int *cell_start;
    dev::GridDesc grid;
    float r2;                     // search radius^2 of THIS pass (the first pass of a two-pass search: (radius / reach)^2)
    int reach;                    // > 1: two-pass search — rows that come back short are searched again with r2_full over a
    float r2_full;                //      stencil `reach` cells wide (nn_wide_kernel) ...
    int *short_list;              // when short_count is given: the rows of handed-over workgroups (and the short rows of a two-pass
    unsigned *short_count;        //      search) are listed here [ns] + counted and nn_wide_kernel searches them; there is no cleanup
                                  //      launch then
    unsigned *short_next;         // the other counter of that list's ping-pong pair (nullable): every launch leaves it at zero
    unsigned *short_seen;         // diagnostic: the count nn_wide_kernel saw
    const dev::GridLevel *levels; // multi-level search (n_levels > 1; needs short_count): the level table in device memory,
    int n_levels, base_level;     //      ascending r2_cap; tgt / cell_start / grid above are the base level's
    float r2_cap[dev::kMaxLevels]; //     the levels' r2_cap (host copy of the table's column)
    const unsigned short *level_in;   //  per block and half: the feedback words the previous launch left (UnansweredRows::level_in) ...
    unsigned short *level_out;        //  ... and where this launch leaves its own [2 x blocks of 256 queries each]
    unsigned *level_dbg;          //      diagnostic counters (nullable)
    int m;                        // max_neighbours (<= the M of the variant that is called)
    int *nbr, *cnt;               // the ELL association [m][ns], [ns]
    unsigned *dm2;                // per query: float bits of its m-th neighbour's d2 (the temporal cut-off)
    int dm2_in;                   // dm2 of the previous association is usable
    unsigned long long *stamps;   // diagnostic build only (nullptr otherwise)
    int *ovf_list;                // workgroups handed to the cleanup kernel by this launch ...
    unsigned *ovf_now, *ovf_next; // ... counted here; the other counter of the ping-pong pair
    unsigned char *split_flag;    // the split table (see SplitTable)
    int *split_list;
    unsigned *split_state;        // {registrations, registrations visible to extra workgroups}
    dev::PendingMove pm;
    dev::VerletLists verlet;        // steady-state Verlet lists (buffers of [16][ns] + per-row state), used when verlet_mode != 0:
    int verlet_mode;                //   0 off; 1 this association builds every row's list; 2 workgroups whose rows' lists still
                                    //   hold answer from them, the others search and rebuild
    const dev::FusedMoments *fuse;  // the pose / model of the K23 the plan folds into K1 (plan.fused)
    const dev::FoldSolve *fold;     // ... and the fold-and-solve step that rides in the cleanup launch (plan.merged)
    dev::LoopState *loop_st;        // device-paced loop: every launch steps aside while its abort flag is up (nullable)
    void (*between)(void *);        // called between the two launches (profiling scopes), may be null
    void (*between2)(void *);       // ... and before the second pass of a two-pass search
    void *between_arg;
};

// One entry per compiled-in list width (register list of the selection); defined in ppcr_nn_tile.hip.
__attribute__((visibility("hidden"))) void launch_tile_m4(TileLaunch &t);
__attribute__((visibility("hidden"))) void launch_tile_m5(TileLaunch &t);
__attribute__((visibility("hidden"))) void launch_tile_m8(TileLaunch &t);
__attribute__((visibility("hidden"))) void launch_tile_m10(TileLaunch &t);
__attribute__((visibility("hidden"))) void launch_tile_m16(TileLaunch &t);
__attribute__((visibility("hidden"))) void launch_tile_m20(TileLaunch &t);
__attribute__((visibility("hidden"))) void launch_tile_m32(TileLaunch &t);

}  // namespace ppcr
