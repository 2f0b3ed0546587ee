// K1 launches for ONE compiled-in list width M (-DPPCR_TILE_M=<4|5|8|10|16|20|32>): the build compiles this file once
// per width, in parallel — the instantiations of nn_fast_kernel / nn_tile_cleanup_kernel are most of the library's
// compile time.  Host code here only launches what the caller's plan names; the C-ABI translation unit (ppcr_hip.hip) fills
// the TileLaunch and owns every buffer it names.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "ppcr_nn_tile.hip.h"
#include "ppcr_nn_tile_launch.hip.h"

#ifndef PPCR_TILE_M
#error "compile with -DPPCR_TILE_M=<list width>"
#endif

namespace ppcr {
namespace {

using namespace ppcr::dev;

// nn_fast_kernel over every block, then nn_tile_cleanup_kernel over the blocks the fast flavour handed over (usually
// none: the cleanup launch then costs a few microseconds of an empty grid) or nn_wide_kernel over the rows it listed.
// Which instantiation, on what grid, with which split table: t.plan (ppcr_k1_plan.hpp), made by the caller.
// LDS budget per 256-query block: halo CAP*13 B (x, y, z + a row byte) + list C*512 B (+0.4 KB tables).  With the
// column order of the source typical halos are ~1000-1400 candidates at the benchmark density; the margin keeps
// denser clouds and drifted sources in the fast flavour (measured when the source was ordered in 4x4x4 bricks, fresh /
// drifted: CAP 2048: 249/341 us, 2176: 231/246, 2240: 230/246, 2272: 302/318).
//
// PPCR_LIST_NOCLAMP: every instantiation of nn_fast_kernel this unit can launch — every entry of k1_fast_variants<M>() —
// must own exactly FastLds::kBytes of LDS (see FastLds).  Checked once per process and list width; a mismatch is a build
// defect, not a run-time condition: abort.
template <int M, size_t I>
bool fast_kernel_lds_ok()
{
#if PPCR_LIST_NOCLAMP
    constexpr K1Fast f = k1_fast_variants<M>().v[I];
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&nn_fast_kernel<M, f.C, f.CAP, f.STAMPS, f.FTM, f.MULTI, f.VERLET>)) != hipSuccess) return false;
    // (the Verlet variants: their allocation is the larger of the search's and the list path's)
    return (int)attr.sharedSizeBytes == FastLds<f.C, f.CAP, f.MULTI, ((f.VERLET != 0 && f.FTM != -2) ? M : 0)>::kAllocBytes;
#else
    return true;
#endif
}
template <int M, size_t... I>
void check_fast_kernel_lds(std::index_sequence<I...>)
{
    static const bool ok = (fast_kernel_lds_ok<M, I>() && ...);
    if (!ok) {
        std::fprintf(stderr, "libppcr_hip: nn_fast_kernel<%d, ...> owns LDS besides its FastLds allocation: the unclamped list stores "
                             "would overwrite it (build defect)\n", M);
        std::abort();
    }
}

// launches entry I of k1_fast_variants<M>() if it is the one the plan names
template <int M, size_t I>
bool launch_fast_if(const TileLaunch &t, const SplitTable &split, const FusedMoments &fm, const LoopReset &lr, const UnansweredRows &un,
                    const VerletLists &vv)
{
    constexpr K1Fast f = k1_fast_variants<M>().v[I];
    if (!(f == t.plan.fast)) return false;
    nn_fast_kernel<M, f.C, f.CAP, f.STAMPS, f.FTM, f.MULTI, f.VERLET><<<t.plan.grid, 256, 0, t.stream>>>(
        t.src, t.ns, t.tgt, t.cell_start, t.grid, t.r2, t.m, t.nbr, t.cnt, t.pm, t.dm2, t.dm2_in, t.ovf_list, t.ovf_now, t.ovf_next, split,
        (t.plan.pass_stamps ? t.stamps : nullptr), fm, lr, un, vv);
    return true;
}
template <int M, size_t... I>
bool launch_fast(std::index_sequence<I...>, const TileLaunch &t, const SplitTable &split, const FusedMoments &fm, const LoopReset &lr,
                 const UnansweredRows &un, const VerletLists &vv)
{
    return (launch_fast_if<M, I>(t, split, fm, lr, un, vv) || ...);
}
// ... and entry I of kK1CleanupVariants
// (the cleanup flavour meets neighbourhoods of 50+ in-radius candidates without a cut-off: lists of 64 (one scan and one
//  selection where 32 slots need two or three rescans); 62 KB of LDS: two workgroups per CU for kernels that run on a few
//  workgroups)
template <int M, size_t I>
bool launch_cleanup_if(const TileLaunch &t, const FusedMoments &fm, const FoldSolve &fs)
{
    constexpr K1Cleanup f = kK1CleanupVariants[I];
    if (!(f == t.plan.cleanup)) return false;
    nn_tile_cleanup_kernel<M, 64, 256, k1_first_cap(M), f.FTM, f.MERGE><<<t.plan.cleanup_grid, 256, 0, t.stream>>>(
        t.src, t.ns, t.tgt, t.cell_start, t.grid, t.r2, t.m, t.nbr, t.cnt, t.dm2, t.ovf_list, t.ovf_now, t.split_list, t.plan.cleanup_n_extra, fm, fs);
    return true;
}
template <int M, size_t... I>
bool launch_cleanup(std::index_sequence<I...>, const TileLaunch &t, const FusedMoments &fm, const FoldSolve &fs)
{
    return (launch_cleanup_if<M, I>(t, fm, fs) || ...);
}

[[noreturn]] void no_such_variant(const char *kernel, int M)
{
    std::fprintf(stderr, "libppcr_hip: the K1 plan names an instantiation of %s<%d, ...> that was not compiled (build defect)\n", kernel, M);
    std::abort();
}

template <int M>
void launch_tile(TileLaunch &t)
{
    constexpr auto kFastVariants = std::make_index_sequence<k1_fast_variants<M>().n>();
    check_fast_kernel_lds<M>(kFastVariants);
    const K1Plan &p = t.plan;
    if (p.M != M) no_such_variant("nn_fast_kernel", M);
    const bool table = k1_split_has_table(p.split);
    const SplitTable split{(table ? t.split_flag : nullptr), (table ? t.split_list : nullptr), (table ? t.split_state : nullptr),
                           (table ? t.split_state + 1 : nullptr), k1_split_n_extra(p.split), p.split_cap, (p.split == kSplitTwoPerBlock ? 1 : 0)};
    FusedMoments fm_none;
    std::memset(&fm_none, 0, sizeof(fm_none));
    VerletLists vv_none;
    std::memset(&vv_none, 0, sizeof(vv_none));
    const LoopReset lr{t.loop_st};
    const bool multi = p.fast.MULTI;
    UnansweredRows un{(t.short_count ? t.short_list : nullptr), t.short_count, t.short_next, ((t.reach > 1 || multi) ? t.m : 0),
                      (multi ? t.levels : nullptr), (multi ? t.n_levels : 0), t.base_level, t.r2_full, {},
                      (multi ? t.level_in : nullptr), (multi ? t.level_out : nullptr), (multi ? t.level_dbg : nullptr),
                      (p.list_all ? 1 : 0)};
    for (int l = 0; l < kMaxLevels; l++) un.r2_cap[l] = (multi && l < t.n_levels) ? t.r2_cap[l] : 0.f;
    // Verlet lists (t.verlet_mode: 1 build them in this launch, 2 verify first and rebuild where needed)
    VerletLists vv = vv_none;
    if (p.fast.VERLET != 0) {
        vv = t.verlet;
        vv.build_all = t.verlet_mode == 2 ? 0 : 1;
        if (p.drop_verlet_order) vv.order_now = nullptr, vv.order_next = nullptr, vv.count_now = nullptr, vv.count_next = nullptr, vv.count_clear = nullptr;
    }
    if (!launch_fast<M>(kFastVariants, t, split, (p.fast.FTM != -2 ? *t.fuse : fm_none), lr, un, vv)) no_such_variant("nn_fast_kernel", M);
    if (!p.wide) {
        if (t.between) t.between(t.between_arg);
        FoldSolve fs_none;
        std::memset(&fs_none, 0, sizeof(fs_none));
        fs_none.loop.st = t.loop_st;  // the cleanup role steps aside with everybody else
        FoldSolve fold_now = t.fold ? *t.fold : fs_none;
        fold_now.handed_over = t.ovf_now;  // this launch's counter (the caller toggled the pair after the fold was prepared)
        if (!launch_cleanup<M>(std::make_index_sequence<sizeof(kK1CleanupVariants) / sizeof(kK1CleanupVariants[0])>(), t,
                               (p.cleanup.FTM != -2 ? *t.fuse : fm_none), (p.cleanup.MERGE ? fold_now : fs_none)))
            no_such_variant("nn_tile_cleanup_kernel", M);
        return;
    }
    if (t.between2) t.between2(t.between_arg);
    // the rows the tiled kernel did not answer — those of handed-over workgroups (marked unsearched) and, in a two-pass
    // search, those that came back short — were listed by the kernel itself; they are searched one row per wave, in
    // place of the cleanup launch (nothing is folded in this mode).  A fixed grid of waves strides over the list: its
    // length is only known on the device.
#ifndef PPCR_WIDE_PER_CU
#define PPCR_WIDE_PER_CU 6
#endif
    constexpr int kWideGrid = 256 * PPCR_WIDE_PER_CU;  // six workgroups per CU are resident (74 VGPRs, 22 KB of LDS): 6144 waves, a row each
    // (with Verlet lists in use the rows searched here get theirs; otherwise vl is null and the kernel is the plain search)
    nn_wide_kernel<M><<<kWideGrid, 256, 0, t.stream>>>(t.src, t.ns, t.tgt, t.cell_start, t.grid, t.reach, t.r2, t.r2_full, t.m, t.nbr,
                                                        t.cnt, t.dm2, t.short_list, t.short_count, t.short_seen, t.loop_st,
                                                        (p.verlet_built ? t.verlet : vv_none));
}

}  // namespace

#define PPCR_CAT2(a, b) a##b
#define PPCR_CAT(a, b) PPCR_CAT2(a, b)
void PPCR_CAT(launch_tile_m, PPCR_TILE_M)(TileLaunch &t) { launch_tile<PPCR_TILE_M>(t); }

}  // namespace ppcr
