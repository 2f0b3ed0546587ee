// csrc/ppcr_k1_plan.hpp on the host: every query of the enumeration below, one line "query|plan" each (the pytest compares
// them with tests/golden/k1_plan_table.txt.gz, recorded from launch_tile<M> as it was before the plan existed), and the
// plan's structural invariants.  `--queries` prints the queries alone (what the recording was driven with).
//
// The enumeration is the cross product of
//   m in {1, 4, 5, 7, 8, 10, 11, 16, 20, 21, 32}, blocks in {1, 391, 1017, 3907}, dm2_in, short_lists, stamps,
//   K23 form in {-2, 0, 8, -3}, merge wanted, verlet_mode in {0, 1, 2}, verlet_rows, verlet_big_tile, reach in {1, 3},
//   n_levels in {1, 3}, short list in use, list_all, (quiet, handed_last) in {(1, 0), (0, 3), (0, 200), (0, unknown)}
// thinned to what the old launch_tile could tell apart (the full product is 2.2 M lines, too large to keep): it read
//   the fold only with a K23 form offered          -> merge wanted varies only then,
//   verlet_big_tile only in Verlet mode, verlet_rows only in the small tile -> they vary only with verlet_mode != 0, verlet_rows
//                                                      only without verlet_big_tile,
//   quiet / handed_last only for the cleanup launch -> they vary only without the short list,
//   list_all only with the short list               -> it varies only with it,
//   reach only for the listed rows' width           -> it varies only with the short list (a two-pass search always has one).
#include <cstdio>
#include <cstring>

#include "ppcr_k1_plan.hpp"

using namespace ppcr;

static int failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (failed++ < 20) std::printf("FAILED %s: %s\n", #cond, line);  \
        }                                                                    \
    } while (0)

static void print_query(char *out, const K1Query &q)
{
    std::sprintf(out, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", q.m, q.blocks, q.dm2_in, q.short_lists, q.stamps, q.k23_form,
                 q.merge_wanted, q.verlet_mode, q.verlet_rows, q.verlet_big_tile, q.reach, q.n_levels, q.short_list, q.list_all, q.quiet,
                 q.handed_last == ~0u ? -1 : (int)q.handed_last);
}

// fast: M C CAP STAMPS FTM MULTI VERLET grid; split: table n_extra cap two-per-block; stamps passed; Verlet order dropped;
// second launch: w, or c FTM MERGE grid n_extra; fused merged verlet_built list_all
static void print_plan(char *out, const K1Plan &p)
{
    out += std::sprintf(out, "%d %d %d %d %d %d %d %d  %d %d %d %d  %d %d  ", p.M, p.fast.C, p.fast.CAP, p.fast.STAMPS, p.fast.FTM, p.fast.MULTI,
                        p.fast.VERLET, p.grid, k1_split_has_table(p.split), k1_split_n_extra(p.split), p.split_cap, p.split == kSplitTwoPerBlock,
                        p.pass_stamps, p.drop_verlet_order);
    if (p.wide) out += std::sprintf(out, "w");
    else out += std::sprintf(out, "c %d %d %d %d", p.cleanup.FTM, p.cleanup.MERGE, p.cleanup_grid, p.cleanup_n_extra);
    std::sprintf(out, "  %d %d %d %d", p.fused, p.merged, p.verlet_built, p.list_all);
}

static K1FastList k1_fast_variants_of(int M)
{
    return M == 4 ? k1_fast_variants<4>() : M == 5 ? k1_fast_variants<5>() : M == 8 ? k1_fast_variants<8>() : M == 10 ? k1_fast_variants<10>()
         : M == 16 ? k1_fast_variants<16>() : M == 20 ? k1_fast_variants<20>() : k1_fast_variants<32>();
}

static void check_plan(const K1Query &q, const K1Plan &p, const char *line)
{
    const K1FastList l = k1_fast_variants_of(p.M);
    bool listed = false;
    for (int i = 0; i < l.n; i++) listed = listed || l.v[i] == p.fast;
    CHECK(p.M == k1_width(q.m) && q.m <= p.M);
    CHECK(listed);
    if (!p.wide) {
        bool cleanup_listed = false;
        for (const K1Cleanup &f : kK1CleanupVariants) cleanup_listed = cleanup_listed || f == p.cleanup;
        CHECK(cleanup_listed);
        CHECK(p.cleanup.MERGE == p.merged && p.cleanup.FTM == p.fast.FTM);
        CHECK(p.cleanup_grid >= 1 && p.cleanup_grid <= q.blocks + dev::kNSums);
    }
    CHECK(!p.merged || p.fused);
    CHECK(p.fused == (p.fast.FTM != -2));
    CHECK(!p.fused || (q.m <= 10 && (p.split == kSplitSteady || p.split == kSplitVerlet)));
    CHECK(p.wide == q.short_list);
    CHECK(!p.wide || !p.merged);
    CHECK(p.verlet_built == (p.fast.VERLET != 0));
    CHECK(!p.verlet_built || (k1_has_steady_variant(q) && q.verlet_mode != 0));
    // what associate_impl sizes ovf_list, the Verlet streak bytes (k1_max_grid) and the partial sums (k1_steady_grid) for
    CHECK(p.grid >= q.blocks && p.grid <= k1_max_grid(q.blocks));
    CHECK(!p.fused || p.grid == k1_steady_grid(q.blocks));
    // the caller's forecast of the short list agrees with what the plan then does
    if (q.short_list == k1_wants_short_list(q) && q.n_levels == 1) CHECK(p.fused == k1_can_fuse(q));
}

int main(int argc, char **argv)
{
    const bool queries_only = argc > 1 && std::strcmp(argv[1], "--queries") == 0;
    const int ms[] = {1, 4, 5, 7, 8, 10, 11, 16, 20, 21, 32}, blocks[] = {1, 391, 1017, 3907}, forms[] = {-2, 0, 8, -3};
    const struct { bool quiet; unsigned handed; } last[] = {{true, 0u}, {false, 3u}, {false, 200u}, {false, ~0u}};
    long n = 0;
    char line[512];
    K1Query q{};
    for (int m : ms)
    for (int nb : blocks)
    for (int dm2_in = 0; dm2_in < 2; dm2_in++)
    for (int short_lists = 0; short_lists < 2; short_lists++)
    for (int stamps = 0; stamps < 2; stamps++)
    for (int form : forms)
    for (int merge = 0; merge < (form != -2 ? 2 : 1); merge++)
    for (int vmode = 0; vmode < 3; vmode++)
    for (int vbig = 0; vbig < (vmode ? 2 : 1); vbig++)
    for (int vrows = 0; vrows < ((vmode && !vbig) ? 2 : 1); vrows++)
    for (int n_levels = 1; n_levels <= 3; n_levels += 2)
    for (int short_list = 0; short_list < 2; short_list++)
    for (int reach = 1; reach <= (short_list ? 3 : 1); reach += 2)
    for (int list_all = 0; list_all < (short_list ? 2 : 1); list_all++)
    for (int k = 0; k < (short_list ? 1 : 4); k++) {
        q.m = m, q.blocks = nb, q.dm2_in = dm2_in, q.short_lists = short_lists, q.stamps = stamps, q.k23_form = form, q.merge_wanted = merge;
        q.verlet_mode = vmode, q.verlet_rows = vrows, q.verlet_big_tile = vbig, q.reach = reach, q.n_levels = n_levels;
        q.short_list = short_list, q.list_all = list_all, q.quiet = last[k].quiet, q.handed_last = last[k].handed;
        print_query(line, q);
        if (!queries_only) {
            const K1Plan p = plan_k1(q);
            char *at = line + std::strlen(line);
            *at++ = '|';
            print_plan(at, p);
            check_plan(q, p, line);
        }
        std::puts(line);
        n++;
    }
    if (!queries_only) std::printf("k1 plan test: %ld queries, %d failed\n", n, failed);
    return failed ? 1 : 0;
}
