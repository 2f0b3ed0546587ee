// The plan of one K1 (nn_fast_kernel + its second launch): which instantiation runs, on what grid, with which split table,
// and what follows it.  Host logic only — no HIP include, compiles with plain g++ (tests/cpp/test_k1_plan.cc) — and the ONE
// place that decides: associate_impl (ppcr_hip_iteration.inc) fills a K1Query and sizes its buffers from the K1Plan,
// launch_tile<M> (ppcr_nn_tile.hip) launches what the plan names and instantiates what k1_fast_variants<M>() lists.
#pragma once
#include <algorithm>
#include <climits>

namespace ppcr {
namespace dev {

constexpr int kNSums = 19;
constexpr int kMaxSplit = 128;  // K1: blocks that can be scanned as two half-blocks (SplitTable in ppcr_nn_tile.hip.h)

#ifndef PPCR_VERLET_SLOTS
#define PPCR_VERLET_SLOTS 16
#endif
// list slots per row by the association's compiled-in width M (10 neighbours: 16 slots hold the ~13.5 targets a list's reach
// holds at the benchmark's density; the command line's 20: 32), and the LDS list slots of the search that builds the lists
constexpr int verlet_slots(int M) { return M <= 12 ? PPCR_VERLET_SLOTS : 32; }
constexpr int verlet_scan_slots(int M) { return M <= 12 ? (PPCR_VERLET_SLOTS <= 16 ? 24 : 28) : 36; }

}  // namespace dev

// Halo capacity of the steady-state (16-slot) variant: 31.3 KB of LDS, five workgroups per CU (1792: four).
constexpr int kCapSteady = 1728;
// ... of the Verlet variant (four workgroups per CU either way: its list path holds 48 coordinates in registers), whose
// lists reach further than the plain search's cut-off: larger cells, larger halos
constexpr int kCapVerlet = 1920;
// ... and of that variant where the cloud is denser (a block's halo outgrows 1920 candidates for more blocks than can be split):
// the first association's 2240-candidate tile, three workgroups per CU (K1Query::verlet_big_tile)
constexpr int kCapVerletBig = 2240;
// ... and of the Verlet variant of the mid-width lists (the command line's 20 neighbours: 32-slot Verlet lists, 36-slot scan
// lists — 18.9 KB — beside the halo: 1600 candidates keep the kernel at four workgroups per CU)
constexpr int kCapVerletMid = 1600;

// The compiled-in list width that serves max_neighbours m (the K1 translation unit is compiled once per width).
constexpr int k1_width(int m) { return m <= 4 ? 4 : m <= 5 ? 5 : m <= 8 ? 8 : m <= 10 ? 10 : m <= 16 ? 16 : m <= 20 ? 20 : 32; }
// The first association's variant (no cut-off yet): 32-slot lists and the 2240-candidate tile, three workgroups per CU.
constexpr int k1_first_slots(int M) { return M <= 24 ? 32 : 48; }
constexpr int k1_first_cap(int M) { return M <= 24 ? 2240 : 2048; }
// Mid-width lists (12 < M <= 24: the command line's 20 neighbours) have a steady-state variant of their own: with the
// temporal cut-off the lists end near m entries, so 24 / 28 slots do (an overflowing lane tightens its threshold and
// scans again), and with a 2048- / 1920-candidate halo the kernel takes ~40 KB of LDS: FOUR workgroups per CU instead
// of three.  200k points are 782 blocks: three per CU run them in two residency rounds (768 slots), four in one.
constexpr bool k1_is_mid(int M) { return M > 12 && M <= 24; }
constexpr int k1_mid_slots(int M) { return M <= 16 ? 24 : 28; }
constexpr int k1_mid_cap(int M) { return M <= 16 ? 2048 : 1920; }
// a block registers for splitting once its halo passes 15/16 of the tile
constexpr int k1_split_cap(int cap) { return cap * 15 / 16; }

// workgroups (= partial-sum slots when K23 is folded in) of a steady-state K1 launch over nb blocks of 256 queries
constexpr int k1_steady_grid(int nb) { return nb + dev::kMaxSplit; }
// ... of a multi-level search: two workgroups per block (the second only works for blocks marked split), in groups of eight
constexpr int k1_two_per_block_grid(int nb) { return 2 * ((nb + 7) & ~7); }
// ... and the largest grid any variant launches: ovf_list, the Verlet streak bytes and the stamps are sized for it
constexpr int k1_max_grid(int nb) { return k1_steady_grid(nb) > k1_two_per_block_grid(nb) ? k1_steady_grid(nb) : k1_two_per_block_grid(nb); }

// nn_fast_kernel's template arguments after M
struct K1Fast { int C, CAP; bool STAMPS; int FTM; bool MULTI; int VERLET; };
constexpr bool operator==(const K1Fast &a, const K1Fast &b)
{
    return a.C == b.C && a.CAP == b.CAP && a.STAMPS == b.STAMPS && a.FTM == b.FTM && a.MULTI == b.MULTI && a.VERLET == b.VERLET;
}

// The K23 forms K1 can fold in: none, Gaussian, t with v + dim = 8, t with another integer v + dim.
constexpr int kK1Forms[4] = {-2, 8, 0, -3};

// Every instantiation of nn_fast_kernel that exists for width M: what gets compiled, what the LDS check walks, what a plan
// may name.  Nothing else says so.
struct K1FastList { K1Fast v[24]; int n; };
template <int M>
constexpr K1FastList k1_fast_variants()
{
    constexpr int C = k1_first_slots(M), CAP = k1_first_cap(M), VS = dev::verlet_scan_slots(M);
    K1FastList l{};
    auto add = [&l](K1Fast f) { l.v[l.n++] = f; };
    // the first association, and the multi-level search (which keeps 32 slots and the large tile)
    add({C, CAP, false, -2, false, 0});
    add({C, CAP, false, -2, true, 0});
    // Verlet lists in a multi-level search
    if (M <= 24) add({VS, (M <= 12 ? kCapVerlet : CAP), false, -2, true, 1});
    if (k1_is_mid(M)) {
        add({k1_mid_slots(M), k1_mid_cap(M), false, -2, false, 0});
        add({VS, kCapVerletMid, false, -2, false, 1});
        add({VS, CAP, false, -2, false, 1});  // (the launch that builds every list)
    }
    if (M <= 12) {
        // steady state, with each K23 form folded in; its multi-level flavour
        for (int ftm : kK1Forms) add({16, kCapSteady, false, ftm, false, 0});
        add({16, kCapSteady, false, -2, true, 0});
        // the Verlet variants: plain, rebuilding a few failing rows inside the workgroup, and in the large tile
        for (int ftm : kK1Forms) add({VS, kCapVerlet, false, ftm, false, 1});
        for (int ftm : kK1Forms) add({VS, kCapVerlet, false, ftm, false, 2});
        for (int ftm : kK1Forms) add({VS, kCapVerletBig, false, ftm, false, 1});
    }
    // the diagnostic (option "stamps") instantiations
    if (M == 10) {
        add({16, kCapSteady, true, -2, true, 0});
        add({16, kCapSteady, true, -2, false, 0});
        add({C, CAP, true, -2, false, 0});
    }
    if (M == 10 || M == 20) add({C, CAP, true, -2, true, 0});
    return l;
}
// nn_tile_cleanup_kernel's (FTM, MERGE) forms
struct K1Cleanup { int FTM; bool MERGE; };
constexpr bool operator==(const K1Cleanup &a, const K1Cleanup &b) { return a.FTM == b.FTM && a.MERGE == b.MERGE; }
constexpr K1Cleanup kK1CleanupVariants[7] = {{0, true}, {8, true}, {-3, true}, {0, false}, {8, false}, {-3, false}, {-2, false}};

// What the choice depends on, and nothing else.
struct K1Query {
    int m;                 // max_neighbours
    int blocks;            // 256-query blocks of the source
    bool dm2_in;           // the previous association's cut-offs are usable
    bool short_lists;      // option short_lists
    bool stamps;           // diagnostic build of the kernel asked for (option stamps)
    int k23_form;          // the K23 form offered for folding in: -2 none, 0, 8, -3
    bool merge_wanted;     // ... and the fold-and-solve step may ride in the cleanup launch (option merge_fold and a ticket)
    int verlet_mode;       // 0 off; 1 this association builds every row's list; 2 answer from the lists that still hold
    bool verlet_rows;      // widths up to 10: rebuild a few failing rows inside the workgroup (grids resident all at once)
    bool verlet_big_tile;  // widths up to 10: the 2240-candidate tile (denser clouds)
    int reach;             // > 1: two-pass search
    int n_levels;          // > 1: multi-level search (needs the short-row list)
    bool short_list;       // unanswered rows are listed and nn_wide_kernel searches them (k1_wants_short_list)
    bool list_all;         // try no tile, list every row
    bool quiet;            // the last association this handle heard from handed nothing over
    unsigned handed_last;  // ... how many workgroups it handed over (~0u: not known)
};

// the split table nn_fast_kernel gets
enum K1Split {
    kSplitSteady,       // acts on the table and extends it; a block registers at the steady-state tile's capacity
    kSplitVerlet,       // ... at the Verlet tile's (small or big)
    kSplitMid,          // ... at the mid-width tile's (plain or Verlet)
    kSplitExtendOnly,   // the first association only extends the table: blocks already close to the steady-state capacity
    kSplitNone,         // width 32: no steady-state variant to split for
    kSplitTwoPerBlock,  // multi-level search: no table, the second workgroup of a block works where the block is marked split
};
// ... as the fields of the kernel's SplitTable: the table's buffers are handed over, the extra workgroups in front of the grid
constexpr bool k1_split_has_table(K1Split s) { return s != kSplitNone && s != kSplitTwoPerBlock; }
constexpr int k1_split_n_extra(K1Split s) { return (s == kSplitSteady || s == kSplitVerlet || s == kSplitMid) ? dev::kMaxSplit : 0; }

struct K1Plan {
    int M;                  // the compiled-in width: which launch_tile_m<M> runs
    K1Fast fast;
    int grid;
    K1Split split;
    int split_cap;          // the halo size at which a block registers (INT_MAX: never)
    bool pass_stamps;       // the kernel receives the stamps pointer (with stamps on and M != 10 a non-stamps instantiation does too)
    bool drop_verlet_order; // multi-level search: the two-workgroups-per-block grid is not the one the dispatch order was sized for
    bool wide;              // second launch: nn_wide_kernel over the listed rows; otherwise nn_tile_cleanup_kernel<cleanup>
    K1Cleanup cleanup;
    int cleanup_grid, cleanup_n_extra;
    bool fused, merged;     // K23 was folded into the fast kernel; the fold-and-solve step into the cleanup launch
    bool verlet_built;      // the launch writes / keeps Verlet lists
    bool list_all;          // the kernel tries no tile and lists every row (only with the short-row list)
};

// This width and state has a steady-state variant (widths up to 20, a valid cut-off, short lists, no stamps): Verlet lists
// are only ever built by one ...
inline bool k1_has_steady_variant(const K1Query &q) { return q.m <= 20 && q.dm2_in && q.short_lists && !q.stamps; }
// ... and K23 can only be folded in by that of the widths up to 10
inline bool k1_can_fuse(const K1Query &q) { return q.k23_form != -2 && q.m <= 10 && k1_has_steady_variant(q); }
// Who redoes the rows of handed-over workgroups: the cleanup role of the second launch when K23 is folded in (it folds K23
// for them as well, but walks a dense neighbourhood one candidate per lane at a time), nn_wide_kernel over the short-row
// list otherwise — every launch that cannot fold, every two-pass and multi-level search (an idle nn_wide_kernel costs what
// an idle cleanup launch costs, and the choice does not depend on when a hand-over count reaches the host).
inline bool k1_wants_short_list(const K1Query &q) { return q.reach > 1 || q.n_levels > 1 || !k1_can_fuse(q); }

inline K1Plan plan_k1(const K1Query &q)
{
    const int M = k1_width(q.m), nb = q.blocks;
    const int C = k1_first_slots(M), CAP = k1_first_cap(M), VS = dev::verlet_scan_slots(M);
    const bool cut_off = q.dm2_in && q.short_lists;
    // (one-pass search: only rows marked unsearched are listed, its short rows are final)
    const bool multi = q.n_levels > 1 && q.short_list;
    K1Plan p{};
    p.M = M;
    int ftm = -2;  // model folded into this launch (-2: none)
    bool steady = false;
    if (multi) {
        // multi-level search: every block picks its level of the grid in the kernel; no split table (a block whose halo
        // does not fit at its level leaves its rows to nn_wide_kernel), nothing folded in
        p.grid = k1_two_per_block_grid(nb);
        p.split = kSplitTwoPerBlock, p.split_cap = INT_MAX;
        if (M == 10 && q.stamps && cut_off) {  // diagnostic builds (option stamps): per-phase cycle counts of the multi-level kernel
            p.fast = {16, kCapSteady, true, -2, true, 0};
            p.pass_stamps = true;
        } else if ((M == 10 || M == 20) && q.stamps) {
            p.fast = {C, CAP, true, -2, true, 0};
            p.pass_stamps = true;
        } else if (M <= 24 && !q.stamps && q.verlet_mode != 0 && cut_off) {
            // Verlet lists in a multi-level search: every level's scan builds the lists of the rows whose reach its stencil
            // covers (in base positions: to_base), nn_wide_kernel those of the rows it searches; a block whose rows' lists all
            // hold — or all but a few: see the kernel — picks no level at all.
            p.fast = {VS, (M <= 12 ? kCapVerlet : CAP), false, -2, true, 1};
            p.drop_verlet_order = true;
            p.verlet_built = true;
        } else if (M <= 12 && cut_off) {
            p.fast = {16, kCapSteady, false, -2, true, 0};
        } else {
            // (the mid-width steady-state variant — 28 slots, four workgroups per CU — was measured here as well: rows that search
            //  a level's whole radius accept more than 28 candidates more often, overflow twice and go to nn_wide_kernel: 3.92 k
            //  against 4.07 k it/s on the LiDAR-like scene, 4.13 k against 4.44 k on the slab.  Multi-level searches keep 32 slots.)
            // (32-slot lists with the steady-state halo capacity — 39.4 KB, four workgroups per CU, one residency round for a
            //  200k-point cloud instead of two — were measured: K1 145 -> 128 us on the LiDAR-like scene, 118 -> 92 us on the
            //  slab, but 30-80 % more rows in nn_wide_kernel (more blocks outgrow the smaller tile and cascade): 4.09 k against
            //  3.99 k and 4.17 k against 4.47 k it/s.  The large tile stays.)
            p.fast = {C, CAP, false, -2, true, 0};
        }
        steady = true;
    } else if (M <= 12 && cut_off) {
        // steady state: the temporal cut-off keeps every list near m entries, so half the list capacity does (an
        // overflowing lane tightens its threshold and scans again); a halo capacity that gives FIVE workgroups per CU,
        // and the few blocks that outgrow it are split
        steady = true;
        if (q.k23_form != -2 && !q.stamps) ftm = q.k23_form;
        p.grid = k1_steady_grid(nb);
        if (q.verlet_mode != 0 && !q.stamps) {
            // Verlet lists: answers from the lists where they still hold
            // (verlet_rows: the variant that rebuilds a few failing rows inside the workgroup — grids resident all at once;
            //  verlet_big_tile: denser clouds, whose blocks' halos outgrow the 1920-candidate tile but not the 2240-candidate
            //  one — three workgroups per CU instead of four, which costs the timed windows 2-3 % where the small tile does:
            //  kCapVerlet stays the default)
            const int cap = q.verlet_big_tile ? kCapVerletBig : kCapVerlet;
            p.fast = {VS, cap, false, ftm, false, (!q.verlet_big_tile && q.verlet_rows) ? 2 : 1};
            p.split = kSplitVerlet, p.split_cap = k1_split_cap(cap);
            p.verlet_built = true;
        } else {
            p.fast = {16, kCapSteady, M == 10 && q.stamps, ftm, false, 0};
            p.split = kSplitSteady, p.split_cap = k1_split_cap(kCapSteady);
            p.pass_stamps = q.stamps;
        }
        p.fused = ftm != -2;
    } else if (k1_is_mid(M) && cut_off && q.short_list) {
        steady = true;
        p.grid = k1_steady_grid(nb);
        p.split = kSplitMid;
        if (q.verlet_mode != 0 && !q.stamps) {
            // Verlet lists (32 slots): rows are answered from their lists where those still hold; the rows this launch
            // leaves unanswered — short rows of a two-pass search, a few failing rows of an answering workgroup — are
            // searched AND given fresh lists by nn_wide_kernel
            // (the launch that BUILDS every list scans with the lists' reach in place of the rows' cut-offs: wider x
            //  windows, larger halos — in the 1600-candidate tile a fifth of a 200k cloud's blocks were handed over
            //  there (43 k rows for nn_wide_kernel, 120-200 us).  It runs once per registration: the 2240-candidate
            //  tile, three workgroups per CU.)
            p.fast = {VS, (q.verlet_mode == 1 ? CAP : kCapVerletMid), false, -2, false, 1};
            p.split_cap = k1_split_cap(kCapVerletMid);
            p.verlet_built = true;
        } else {
            p.fast = {k1_mid_slots(M), k1_mid_cap(M), false, -2, false, 0};
            p.split_cap = k1_split_cap(k1_mid_cap(M));
        }
    }
    if (!steady) {
        // the first association (32 slots, three workgroups per CU) keeps the large tile and only extends the split table
        p.fast = {C, CAP, M == 10 && q.stamps, -2, false, 0};
        p.grid = nb;
        p.pass_stamps = q.stamps;
        if (M <= 24) p.split = kSplitExtendOnly, p.split_cap = k1_split_cap(k1_is_mid(M) ? k1_mid_cap(M) : kCapSteady);
        else p.split = kSplitNone, p.split_cap = INT_MAX;
    }
    p.wide = q.short_list;
    p.list_all = q.list_all && q.short_list;
    if (!p.wide) {
        // persistent workgroups over the hand-over list: few when the last association this handle heard from handed nothing
        // over (a handful of hand-overs — a registration that still moves a few per cent of the radius per iteration leaves one
        // to three per launch — do not need 512 workgroups that read a counter and leave: four per workgroup the last launch
        // handed over)
        const int wgs = q.quiet ? std::min(nb, 32)
                                : std::min(nb, (q.handed_last != ~0u && q.handed_last < 128u) ? std::max(32, 4 * (int)q.handed_last) : 512);
        p.merged = ftm != -2 && q.merge_wanted;
        p.cleanup = {ftm, p.merged};
        p.cleanup_grid = wgs + (p.merged ? dev::kNSums : 0);
        p.cleanup_n_extra = steady ? dev::kMaxSplit : 0;
    }
    return p;
}

}  // namespace ppcr
