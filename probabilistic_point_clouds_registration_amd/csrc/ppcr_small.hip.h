// Batches of small cloud pairs (ppcr_batch_run_small, include/ppcr.h): the kernel.  One workgroup of 256 lanes registers one
// pair from its first association to its last transform — search, weights, moments, fold, solve, stopping rule and the move
// of the source all happen inside the workgroup, and nothing leaves the CU but the per-iteration records.
//
//   small_align_kernel<M, TM>   grid: one workgroup per pair.  M: the compiled-in list width (10 / 20; the cut is applied at
//                               max_neighbours at run time), TM: the model, as refine_search_kernel has it.
//
// An outer iteration of a pair.  The source lives in the launch's packed buffer (xyz, 12 bytes a point) and is moved IN PLACE,
// f64 arithmetic and f32 store (move_point), by the step the previous iteration solved, as its lanes load their rows: the
// arithmetic of ppcr_apply_transform, so the numbers are those of ppcr_align.  The search is brute force and exact: the
// target goes through LDS in tiles of kSmallTile points (SoA x / y / z; the original index of a point is tile base +
// position: no index array, no sort), a lane keeps its row in registers and walks the tile — every lane reads the same LDS
// word, a broadcast — and offers what lies inside the radius to its private list with refine_offer / refine_select
// (ppcr_refine.hip.h): the same (d^2, original index) order and the same ties as everywhere else in the library.
//
// Loop order: CHUNKS of 256 rows outside, tiles inside, the tile staged again from L2 for every chunk.  The other order (a
// tile staged once, all chunks walked under it) would have to park the chunks' lists in device memory between tiles: 64 bytes
// a row, written and read once per tile.  Staging a tile again costs 12 bytes a point for 256 rows that then spend ~10
// instructions each on every one of its points: under 1 % of the scan.  And when the whole target fits one tile — every
// cloud up to kSmallTile points, the case this entry point is for — it is staged ONCE per registration and stays.
// LDS: tile 36 KB + lists 16 KB + the fold's 21.3 KB + the solve lane's state 0.6 KB = 74 KB: two workgroups per CU
// (a 96 KB tile for 8192 points would leave one, and the second workgroup is what hides a lane's list compactions).
//
// A list entry is the target's ORIGINAL index (16 bits: at most PPCR_SMALL_MAX_POINTS points).  The selection and the
// moments read an entry's coordinates from the tile when the entry lies in the tile that is staged, from the packed buffer
// otherwise (an entry of an earlier tile of a target of several tiles): the same three floats either way.
//
// The first IRLS step is fused with the search (RowMoments<TM> about the centre of the target's box, at the pose q0 / t0).
// With inner_steps > 1 every row's winners also go to device memory as u16 indices, [max_neighbours][n_source] per pair
// (0xFFFF: no entry), and the later steps stream them: weights and moments at the step's pose, fold, solve, until inner_steps
// or the relative cost decrease is <= f_tol (the test of ppcr_solve / po_solve).  inner_steps == 1 writes nothing.
//
// Every lane adds its rows' moments chunk after chunk in registers and the workgroup folds them once per step
// (block_reduce_store): a fixed order, so a pair's bits depend on nothing but that pair.  One lane then solves
// (solve_rigid_device), composes T_cum <- T_step T_cum in f64, evaluates the stopping rule (small_rule_check below) and
// tells the others through LDS what comes next.  Every loop is bounded by a launch argument (n_iter, inner_steps, chunks,
// tiles): no flags, no global atomics, no waiting on anybody.
#pragma once
#include "ppcr.h"
#include "ppcr_device.hip.h"
#include "ppcr_refine.hip.h"

namespace ppcr {
namespace dev {

constexpr int kSmallTile = 3072;  // target points of a staged tile: 36 KB of LDS as SoA x / y / z
constexpr unsigned short kSmallNone = 0xFFFFu;  // an unused slot of a row's stored winners
static_assert(PPCR_SMALL_MAX_POINTS < 0xFFFF, "list entries and stored winners are 16-bit original indices");

struct SmallPair {  // one pair of a launch: where its clouds lie in the packed buffer (in floats) and its winners (in u16)
    unsigned long long src_off, tgt_off, nbr_off;
    int ns, nt;
    double c[3];  // origin of the moments: the centre of the target's box
};

struct SmallArgs {
    float *packed;
    const SmallPair *pairs;
    unsigned short *nbr;  // nullptr when inner_steps == 1
    long long first;      // index of the launch's first pair in the batch (the outputs are the batch's)
    double *T_out;        // [pair][12]
    int *done_out;        // [pair]
    double *history;      // [pair][n_iter][12], nullable
    double *costs;        // [pair][n_iter][2], nullable
    int *steps;           // [pair][n_iter], nullable
    float r2;
    int m, n_iter, inner_steps;
    double f_tol, thresh, patience;
    double R0[9], t0[3];  // the pose every outer iteration's inner loop starts from (q0 / t0)
    Model md;
};

// the staged tile, the packed target behind it, and a lane's list of original indices
struct SmallCands {
    const float *sx, *sy, *sz;
    const float *tgt;
    unsigned short *list;  // [slot * kBlock + tid]
    int base, len, tid;
    __device__ __forceinline__ float4 get(int e) const
    {
        const unsigned k = (unsigned)(e - base);
        if (k < (unsigned)len) return make_float4(sx[k], sy[k], sz[k], 0.f);
        const float *p = tgt + 3 * (size_t)e;
        return make_float4(p[0], p[1], p[2], 0.f);
    }
    __device__ __forceinline__ unsigned orig_of(int e) const { return (unsigned)e; }
    __device__ __forceinline__ int load(int t) const { return list[t * kBlock + tid]; }
    __device__ __forceinline__ void store(int t, int e) const { list[t * kBlock + tid] = (unsigned short)e; }
};

// hasConverged(): the arithmetic of ppcr_stop_rule_check (ppcr_hip_api.inc), restated for the device with its quirks — the
// drop starts at 0, so the first check counts as idle; a NaN drop fails the comparison and resets the count.  true: go on.
struct SmallRule {
    int iteration, idle;
    double cost_drop;
};
__device__ __forceinline__ bool small_rule_check(SmallRule &r, int n_iter, double thresh, double patience)
{
    if (r.iteration == n_iter) return false;
    if (!(r.cost_drop < thresh)) {
        r.idle = 0;
        return true;
    }
    if ((double)r.idle > patience) return false;
    r.idle += 1;
    return true;
}

template <int M, int TM>
PPCR_SCORE_KERNEL __global__ __launch_bounds__(kBlock) void small_align_kernel(SmallArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_tile[3 * kSmallTile];
    __shared__ unsigned short s_list[kRefineList * kBlock];
    __shared__ double s_S[kNSums];
    __shared__ double s_pose[12];  // [R | t] row-major: the pose of the step being accumulated
    __shared__ double s_move[12];  // the step the previous outer iteration solved: the source's pending move
    __shared__ double s_Tcum[12];  // (the solve lane's)
    __shared__ SmallRule s_rule;   // (the solve lane's)
    __shared__ double s_cost_init;
    __shared__ int s_go;           // what the solve lane decided: 0 stop, 1 another inner step, 2 the next outer iteration

    const int tid = threadIdx.x;
    const SmallPair pr = a.pairs[blockIdx.x];
    const size_t pair = (size_t)a.first + blockIdx.x;
    float *const src = a.packed + pr.src_off;
    const float *const tgt = a.packed + pr.tgt_off;
    unsigned short *const nbr = a.nbr != nullptr ? a.nbr + pr.nbr_off : nullptr;
    const int ns = pr.ns, nt = pr.nt, m = a.m;
    const int nchunks = (ns + kBlock - 1) / kBlock, ntiles = (nt + kSmallTile - 1) / kSmallTile;
    const unsigned r2_bits = __float_as_uint(a.r2);
    float *const sx = s_tile, *const sy = s_tile + kSmallTile, *const sz = s_tile + 2 * kSmallTile;

    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) s_Tcum[k] = (k % 5 == 0) ? 1.0 : 0.0;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int k = 0; k < 3; k++) s_pose[4 * r + k] = a.R0[3 * r + k];
            s_pose[4 * r + 3] = a.t0[r];
        }
        SmallRule rule = {0, 0, 0.0};
        s_go = small_rule_check(rule, a.n_iter, a.thresh, a.patience) ? 2 : 0;
        s_rule = rule;
    }
    __syncthreads();

    bool staged = false;  // (uniform) the target's only tile is in LDS
    for (int it = 0; it < a.n_iter; it++) {
        if (s_go == 0) break;  // (uniform: written before the last barrier)
        for (int step = 1; step <= a.inner_steps; step++) {
            Pose P;  // the step's pose, about the pair's origin
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int k = 0; k < 3; k++) P.R[3 * r + k] = s_pose[4 * r + k];
                P.t[r] = s_pose[4 * r + 3];
                P.c[r] = pr.c[r];
            }
            RowAcc acc;
#pragma unroll
            for (int j = 0; j < kNSums; j++) acc.a[j] = 0.0;

            for (int ch = 0; ch < nchunks; ch++) {
                const int i = ch * kBlock + tid;
                const bool valid = i < ns;
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                if (valid) q = make_float4(src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], 0.f);
                SmallCands S{sx, sy, sz, tgt, s_list, 0, 0, tid};
                int n = 0;
                if (step == 1) {  // (uniform) the move, the search, the cut
                    if (valid && it > 0) {
                        Pose Mv;
#pragma unroll
                        for (int r = 0; r < 3; r++) {
#pragma unroll
                            for (int k = 0; k < 3; k++) Mv.R[3 * r + k] = s_move[4 * r + k];
                            Mv.t[r] = s_move[4 * r + 3];
                            Mv.c[r] = 0.0;
                        }
                        q = move_point(q, Mv);
                        src[3 * (size_t)i] = q.x, src[3 * (size_t)i + 1] = q.y, src[3 * (size_t)i + 2] = q.z;
                    }
                    unsigned lim = r2_bits;
                    for (int tl = 0; tl < ntiles; tl++) {
                        const int base = tl * kSmallTile, len = min(kSmallTile, nt - base);
                        if (ntiles > 1 || !staged) {  // (uniform)
                            __syncthreads();  // nobody reads the tile that was there
                            for (int f = tid; f < 3 * len; f += kBlock) s_tile[(f % 3) * kSmallTile + f / 3] = tgt[3 * (size_t)base + f];
                            __syncthreads();
                            staged = true;
                        }
                        S.base = base, S.len = len;
                        if (valid) {
                            int k = 0;
                            for (; k + 4 <= len; k += 4) {
                                unsigned b[4];
#pragma unroll
                                for (int u = 0; u < 4; u++)
                                    b[u] = __float_as_uint(dist2_flann(q, make_float4(sx[k + u], sy[k + u], sz[k + u], 0.f)));
                                if (min(min(b[0], b[1]), min(b[2], b[3])) < lim) {
#pragma unroll
                                    for (int u = 0; u < 4; u++) refine_offer<M>(S, q, base + k + u, b[u], n, lim, m);
                                }
                            }
                            for (; k < len; k++)
                                refine_offer<M>(S, q, base + k, __float_as_uint(dist2_flann(q, make_float4(sx[k], sy[k], sz[k], 0.f))), n, lim, m);
                        }
                    }
                    if (valid) {
                        if (n > m) {
                            unsigned T;
                            n = refine_select<M>(S, q, n, m, T);
                        }
                        if (nbr != nullptr)
                            for (int j = 0; j < m; j++) nbr[(size_t)j * ns + i] = j < n ? (unsigned short)S.load(j) : kSmallNone;
                    }
                } else if (valid) {  // a later step: the stored winners, in the order they were stored in
                    S.base = (ntiles - 1) * kSmallTile, S.len = nt - S.base;  // (the tile the search left in LDS)
                    for (; n < m; n++) {
                        const unsigned short e = nbr[(size_t)n * ns + i];
                        if (e == kSmallNone) break;
                        S.store(n, e);
                    }
                }
                if (valid && n > 0) {  // weights and the row's share of the moments at P
                    double xr[3];
                    rotate_point(P, q, xr);
                    RowMoments<TM> row;
                    row.begin(a.md);
#pragma unroll
                    for (int j = 0; j < M; j++) {
                        if (j < n) {
                            const float4 y = S.get(S.load(j));
                            row.add_pair(a.md, xr, y.x, y.y, y.z);
                        }
                    }
                    row.finish(acc, P, q, xr);
                }
            }

            if (tid < kNSums) s_S[tid] = 0.0;  // (the lanes that add to it in the fold)
            block_reduce_store<kBlock, true>(acc, nullptr, 0, 0, s_S);
            __syncthreads();
            if (tid == 0) {
                double Sm[kNSums];
#pragma unroll
                for (int j = 0; j < kNSums; j++) Sm[j] = s_S[j];
                const DeviceSolve rs = solve_rigid_device(static_cast<const double *>(Sm), pr.c);
                // the inner loop's test (solve_impl / po_solve) on the same numbers
                const double cost_old = 0.5 * Sm[16];
                const double fc = rs.degenerate ? cost_old : rs.cost;
                if (step == 1) s_cost_init = cost_old;
                const bool fin = rs.degenerate || step >= a.inner_steps ||
                                 (cost_old - fc) <= fmax(a.f_tol * cost_old, 1e-14 * 0.5 * (Sm[17] + Sm[18]));
                if (!fin) {
#pragma unroll
                    for (int r = 0; r < 3; r++) {
#pragma unroll
                        for (int k = 0; k < 3; k++) s_pose[4 * r + k] = rs.R[3 * r + k];
                        s_pose[4 * r + 3] = rs.t[r];
                    }
                    s_go = 1;
                } else {  // the outer iteration is over: T_cum <- T_step T_cum, the record, the rule
                    double Tn[12];
#pragma unroll
                    for (int r = 0; r < 3; r++) {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            double v = (rs.R[3 * r] * s_Tcum[k] + rs.R[3 * r + 1] * s_Tcum[4 + k]) + rs.R[3 * r + 2] * s_Tcum[8 + k];
                            if (k == 3) v += rs.t[r];
                            Tn[4 * r + k] = v;
                        }
                    }
                    const double c0 = s_cost_init;
#pragma unroll
                    for (int k = 0; k < 12; k++) s_Tcum[k] = Tn[k];
                    const size_t rec = pair * (size_t)a.n_iter + (size_t)it;
                    if (a.history != nullptr)
                        for (int k = 0; k < 12; k++) a.history[rec * 12 + k] = Tn[k];
                    if (a.costs != nullptr) a.costs[rec * 2] = c0, a.costs[rec * 2 + 1] = fc;
                    if (a.steps != nullptr) a.steps[rec] = step;
#pragma unroll
                    for (int r = 0; r < 3; r++) {
#pragma unroll
                        for (int k = 0; k < 3; k++) {
                            s_move[4 * r + k] = rs.R[3 * r + k];
                            s_pose[4 * r + k] = a.R0[3 * r + k];
                        }
                        s_move[4 * r + 3] = rs.t[r];
                        s_pose[4 * r + 3] = a.t0[r];
                    }
                    SmallRule rule = s_rule;
                    rule.cost_drop = (c0 - fc) / c0;  // cc:119
                    rule.iteration++;                 // cc:130
                    s_go = small_rule_check(rule, a.n_iter, a.thresh, a.patience) ? 2 : 0;
                    s_rule = rule;
                }
            }
            __syncthreads();
            if (s_go != 1) break;  // (uniform)
        }
    }
    if (tid == 0) {
        for (int k = 0; k < 12; k++) a.T_out[pair * 12 + k] = s_Tcum[k];
        a.done_out[pair] = s_rule.iteration;
    }
}

}  // namespace dev
}  // namespace ppcr
