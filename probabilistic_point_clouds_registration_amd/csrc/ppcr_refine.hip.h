// Refining many candidate poses of one source against one resident target (ppcr_scorer_refine, include/ppcr.h): the kernels.
//
// One iteration of every pose is two launches on one stream, and the host is not asked anything in between:
//   refine_search_kernel<M, TM>  per (block of 256 source rows, pose): the rows moved by the pose, the radius search with the
//                                max_neighbours cut, the weights and the rows' share of the 19 moments — the association
//                                lives in LDS and registers and never reaches memory;
//   refine_solve_kernel          per pose: the partial moments folded in block order, the closed-form rigid solve, the pose
//                                composed with the step in f64 in device memory, the iteration's record.
//
// The search of one (block, pose).  The source was sorted by the cells of its own box, so a block is spatially compact and a
// rigid move keeps it so.  The block's lanes reduce the cell range their 27-cell stencils cover on the RADIUS grid (cells of
// edge >= radius: not the scorer's nearest-neighbour grid), and every (y, z) row of cells of that range — one contiguous run of
// the cell-sorted target — is staged into LDS once, as SoA x / y / z / original index.  A lane then scans the (up to nine)
// rows of its own stencil from LDS, appends what lies inside the radius to its private list (LDS, [slot][lane]) and cuts the
// list to its m closest by (d^2, original index) with the v_med3_u32 sorted insert (ppcr_device.hip.h), on the spot whenever
// the list fills up and once at the end.  The winners' coordinates come from the tile again for the f64 weights and moments.
// A range that holds more targets than the tile (kRefineTile), or more rows than a workgroup has lanes, takes the second path:
// every lane scans its stencil from global memory (for_each_candidate) into a list of positions that borrows the tile's
// memory; the selection is the same code, so the same rows come out.
//
// Every f64 sum is folded in a fixed order and the pair counts are integers: the same inputs give the same bits, whatever
// other poses share the launch.
#pragma once
#include "ppcr.h"
#include "ppcr_device.hip.h"
#include "ppcr_score.hip.h"

namespace ppcr {
namespace dev {

constexpr int kRefinePosesPerWg = 4;   // poses a workgroup takes in turn, its 256 rows held in registers
constexpr int kRefineTile = 2048;      // candidates of a staged cell range: 32 KB of LDS as SoA x / y / z / index
constexpr int kRefineList = 32;        // slots of a lane's candidate list (> the widest cut, 20: a compaction leaves room)
constexpr int kRefineRows = kBlock;    // (y, z) rows of cells of a staged range: one lane prepares each
constexpr int kRefineSums = kNSums + 1;  // per (pose, block): the 19 partial moments and the pair count (an integer in 8 bytes)
// LDS of refine_search_kernel: tile 32 KB + lists 16 KB + the fold's 21.3 KB + tables 2 KB = 72 KB: two workgroups per CU
static_assert(kRefineList * kBlock * (int)sizeof(int) <= 4 * kRefineTile * (int)sizeof(float), "the second path's list borrows the tile");
static_assert(kRefineTile <= 65536, "list entries of the tiled path are 16-bit tile indices");

// where a lane's candidates come from, and its list of them
struct RefineTileCands {  // the staged range; list entries are tile indices
    const float *sx, *sy, *sz;
    const int *si;
    unsigned short *list;  // [slot * kBlock + tid]
    int tid;
    __device__ __forceinline__ float4 get(int e) const { return make_float4(sx[e], sy[e], sz[e], 0.f); }
    __device__ __forceinline__ unsigned orig_of(int e) const { return (unsigned)si[e]; }
    __device__ __forceinline__ int load(int t) const { return list[t * kBlock + tid]; }
    __device__ __forceinline__ void store(int t, int e) const { list[t * kBlock + tid] = (unsigned short)e; }
};
struct RefineGlobalCands {  // global memory; list entries are positions in the cell-sorted target
    const float4 *tgt;
    int *list;  // [slot * kBlock + tid]
    int tid;
    __device__ __forceinline__ float4 get(int e) const { return tgt[e]; }
    __device__ __forceinline__ unsigned orig_of(int e) const { return (unsigned)__float_as_int(tgt[e].w); }
    __device__ __forceinline__ int load(int t) const { return list[t * kBlock + tid]; }
    __device__ __forceinline__ void store(int t, int e) const { list[t * kBlock + tid] = e; }
};

// A lane's list (n > m entries) cut to its m smallest by (d2, original index), in place; returns the new n (= m) and the
// bit pattern of the m-th smallest d2.  Pass A finds that threshold with the sorted insert, pass B keeps what is not above
// it, and only when more entries tie at the threshold than there is room for do the original indices decide.
template <int M, class S>
__device__ __forceinline__ int refine_select(const S &src, float4 q, int n, int m, unsigned &thr)
{
    unsigned K[M];
#pragma unroll
    for (int j = 0; j < M; j++) K[j] = 0xFFFFFFFFu;
    for (int t = 0; t < n; t++) sorted_insert<M>(K, __float_as_uint(dist2_flann(q, src.get(src.load(t)))));
    const unsigned T = pick<M>(K, m - 1);
    int w = 0, c_eq = 0;
    for (int t = 0; t < n; t++) {
        const int e = src.load(t);
        const unsigned b = __float_as_uint(dist2_flann(q, src.get(e)));
        if (b <= T) {
            src.store(w, e);
            w++;
            c_eq += (b == T) ? 1 : 0;
        }
    }
    if (w > m) {
        const int need = m - (w - c_eq);  // (>= 1: fewer than m entries lie below the m-th smallest)
#pragma unroll
        for (int j = 0; j < M; j++) K[j] = 0xFFFFFFFFu;
        for (int t = 0; t < w; t++) {
            const int e = src.load(t);
            if (__float_as_uint(dist2_flann(q, src.get(e))) == T) sorted_insert<M>(K, src.orig_of(e));
        }
        const unsigned T2 = pick<M>(K, need - 1);
        int w2 = 0;
        for (int t = 0; t < w; t++) {
            const int e = src.load(t);
            const unsigned b = __float_as_uint(dist2_flann(q, src.get(e)));
            if (b < T || src.orig_of(e) <= T2) {
                src.store(w2, e);
                w2++;
            }
        }
        w = w2;
    }
    thr = T;
    return w;
}

// One scanned candidate e with d2 bits b: kept when b < lim.  lim starts as the bits of (float)(r * r) — the strict test of
// the radius search — and drops to (m-th smallest so far) + 1 whenever a full list is compacted: what a compaction drops
// has m entries before it in (d2, index) order for good.
template <int M, class S>
__device__ __forceinline__ void refine_offer(const S &src, float4 q, int e, unsigned b, int &n, unsigned &lim, int m)
{
    if (b < lim) {
        if (n == kRefineList) {
            unsigned T;
            n = refine_select<M>(src, q, n, m, T);
            lim = T + 1u;
            if (!(b < lim)) return;
        }
        src.store(n, e);
        n++;
    }
}

// The row once its scan is over: the cut, then the weights and the row's share of the moments about c (the pose is the
// identity on the moved f32 point q).
template <int M, int TM, class S>
__device__ __forceinline__ int refine_row(const S &src, float4 q, int n, int m, const Model &md, const Pose &P, RowAcc &acc)
{
    if (n > m) {
        unsigned T;
        n = refine_select<M>(src, q, n, m, T);
    }
    if (n > 0) {
        const double xr[3] = {(double)q.x, (double)q.y, (double)q.z};
        RowMoments<TM> row;
        row.begin(md);
#pragma unroll
        for (int j = 0; j < M; j++) {
            if (j < n) {
                const float4 y = src.get(src.load(j));
                row.add_pair(md, xr, y.x, y.y, y.z);
            }
        }
        row.finish(acc, P, q, xr);
    }
    return n;
}

__device__ __forceinline__ int refine_wave_min(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ int refine_wave_max(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// 1. Search, weights and moments.  Grid: (blocks of 256 source rows) x (groups of kRefinePosesPerWg poses).
// partials: [pose][kRefineSums][blocks]; frozen (nullptr in a call's first iteration): poses that found no pair earlier.
// ---------------------------------------------------------------------------------------------------------------------------
template <int M, int TM>
PPCR_SCORE_KERNEL __global__ __launch_bounds__(kBlock) void refine_search_kernel(
    const float4 *__restrict__ src, int ns, const double *__restrict__ poses, const unsigned *__restrict__ frozen, int n_poses,
    const float4 *__restrict__ tgt, const int *__restrict__ cell_start, GridDesc g, ScoreBox box, float radius, float r2, int m,
    Model md, double3 origin, double *__restrict__ partials)
{
    __shared__ float s_tile[4 * kRefineTile];
    __shared__ unsigned short s_list[kRefineList * kBlock];
    __shared__ int s_off[kRefineRows + 1], s_gb[kRefineRows];
    __shared__ int s_range[kBlock / 64][6], s_wtot[kBlock / 64], s_cnt[kBlock / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x, nb = gridDim.x;
    const int i = blk * kBlock + tid;
    const bool valid = i < ns;
    const float4 q0 = valid ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float slack = radius * 1.001f;  // a row farther than this from the target's box on one axis has no pair
    const unsigned r2_bits = __float_as_uint(r2);
    Pose P;
#pragma unroll
    for (int k = 0; k < 9; k++) P.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    P.t[0] = P.t[1] = P.t[2] = 0.0;
    P.c[0] = origin.x, P.c[1] = origin.y, P.c[2] = origin.z;
    float *const sx = s_tile, *const sy = s_tile + kRefineTile, *const sz = s_tile + 2 * kRefineTile;
    int *const si = reinterpret_cast<int *>(s_tile + 3 * kRefineTile);

    const int p_begin = blockIdx.y * kRefinePosesPerWg, p_end = min(p_begin + kRefinePosesPerWg, n_poses);
    for (int p = p_begin; p < p_end; p++) {
        if (frozen != nullptr && frozen[p] != 0u) continue;  // (uniform)
        __syncthreads();  // the previous pose's tile, lists and tables are free
        double *const out = partials + (size_t)p * kRefineSums * nb;
        float qp[3];
        score_move(q0, poses + (size_t)p * 12, qp);
        const float4 q = make_float4(qp[0], qp[1], qp[2], 0.f);
        bool active = valid;
#pragma unroll
        for (int a = 0; a < 3; a++) active = active && qp[a] >= box.lo[a] - slack && qp[a] <= box.hi[a] + slack;  // (NaN: no)
        const QueryCells qc = query_cells(q, g);
        const int cc[3] = {qc.cx, qc.cy, qc.cz};

        // the cell range the active lanes' stencils cover
        int lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = refine_wave_min(active ? cc[a] : INT_MAX);
            hi[a] = refine_wave_max(active ? cc[a] : INT_MIN);
        }
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < 3; a++) s_range[wave][a] = lo[a], s_range[wave][3 + a] = hi[a];
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = s_range[0][a], hi[a] = s_range[0][3 + a];
            for (int w = 1; w < kBlock / 64; w++) lo[a] = min(lo[a], s_range[w][a]), hi[a] = max(hi[a], s_range[w][3 + a]);
        }
        if (lo[0] > hi[0]) {  // (uniform) no row of the block near the target: zeros
            if (tid < kRefineSums) out[(size_t)tid * nb + blk] = 0.0;  // (the count's slot too: all bits zero)
            continue;
        }
#pragma unroll
        for (int a = 0; a < 3; a++) {  // (cc in [-1, n]: lo <= hi holds after the clamps)
            lo[a] = max(lo[a] - 1, 0);
            hi[a] = min(hi[a] + 1, g.n[a] - 1);
        }
        const int ny = hi[1] - lo[1] + 1, nrows = ny * (hi[2] - lo[2] + 1);

        // one contiguous run of the sorted target per (y, z) row of the range: its start, and its place in the tile
        bool tiled = nrows <= kRefineRows;
        if (tiled) {
            int len = 0;
            if (tid < nrows) {
                const int base = ((lo[2] + tid / ny) * g.n[1] + lo[1] + tid % ny) * g.n[0];
                const int b = cell_start[base + lo[0]];
                s_gb[tid] = b;
                len = cell_start[base + hi[0] + 1] - b;
            }
            int inc = len;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(inc, d, 64);
                if (lane >= d) inc += t;
            }
            if (lane == 63) s_wtot[wave] = inc;
            __syncthreads();
            int before = 0, total = 0;
            for (int w = 0; w < kBlock / 64; w++) {
                before += w < wave ? s_wtot[w] : 0;
                total += s_wtot[w];
            }
            if (tid == 0) s_off[0] = 0;
            s_off[tid + 1] = before + inc;
            tiled = total <= kRefineTile;
        }

        RowAcc acc;
#pragma unroll
        for (int j = 0; j < kNSums; j++) acc.a[j] = 0.0;
        int n = 0;
        unsigned lim = r2_bits;
        if (tiled) {  // (uniform)
            __syncthreads();
            for (int r = wave; r < nrows; r += kBlock / 64) {
                const int gb = s_gb[r], off = s_off[r], len = s_off[r + 1] - off;
                for (int k = lane; k < len; k += 64) {
                    const float4 t = tgt[gb + k];
                    sx[off + k] = t.x, sy[off + k] = t.y, sz[off + k] = t.z;
                    si[off + k] = __float_as_int(t.w);
                }
            }
            __syncthreads();
            const RefineTileCands S{sx, sy, sz, si, s_list, tid};
            if (active) {
                for (int dz = -1; dz <= 1; dz++) {
                    const int cz = cc[2] + dz;
                    if (cz < lo[2] || cz > hi[2]) continue;  // (outside the grid)
                    for (int dy = -1; dy <= 1; dy++) {
                        const int cy = cc[1] + dy;
                        if (cy < lo[1] || cy > hi[1]) continue;
                        const int r = (cz - lo[2]) * ny + (cy - lo[1]);
                        const int e1 = s_off[r + 1];
                        for (int e = s_off[r]; e < e1; e++)
                            refine_offer<M>(S, q, e, __float_as_uint(dist2_flann(q, S.get(e))), n, lim, m);
                    }
                }
                n = refine_row<M, TM>(S, q, n, m, md, P, acc);
            }
        } else {
            const RefineGlobalCands S{tgt, reinterpret_cast<int *>(s_tile), tid};
            if (active) {
                for_each_candidate(q, g, cell_start, tgt, [&](int pos, float4 t) {
                    refine_offer<M>(S, q, pos, __float_as_uint(dist2_flann(q, t)), n, lim, m);
                });
                n = refine_row<M, TM>(S, q, n, m, md, P, acc);
            }
        }

        // the block's pair count and its 19 partial moments
        int cnt = active ? n : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
        if (lane == 0) s_cnt[wave] = cnt;
        block_reduce_store<kBlock, true>(acc, out, nb, blk);  // (its barriers also publish s_cnt)
        if (tid == 0) {
            unsigned long long t = 0;
            for (int w = 0; w < kBlock / 64; w++) t += (unsigned long long)s_cnt[w];
            reinterpret_cast<unsigned long long *>(out)[(size_t)kNSums * nb + blk] = t;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// 2. One workgroup per pose: the partials folded in block order, the solve, T <- T_step T in f64, the iteration's record.
// A pose whose association has no weight freezes: it keeps its T, reports zeros, and is left alone from then on.
// ---------------------------------------------------------------------------------------------------------------------------
PPCR_SCORE_KERNEL __global__ __launch_bounds__(kBlock) void refine_solve_kernel(const double *__restrict__ partials, int nb,
                                                                                 double3 origin, double *__restrict__ poses,
                                                                                 unsigned *__restrict__ frozen, int first,
                                                                                 ppcr_pose_step *__restrict__ out)
{
    __shared__ double s_w[kBlock / 64];
    __shared__ double s_S[kNSums];
    __shared__ unsigned long long s_pairs;
    const int p = blockIdx.x, tid = threadIdx.x;
    double *const T = poses + (size_t)p * 12;
    ppcr_pose_step rec;
#pragma unroll
    for (int k = 0; k < 12; k++) rec.T[k] = 0.0;
    rec.cost[0] = rec.cost[1] = 0.0;
    rec.weight_sum = 0.0;
    rec.n_pairs = 0;
    if (!first && frozen[p] != 0u) {  // (uniform)
        if (tid == 0) {
            for (int k = 0; k < 12; k++) rec.T[k] = T[k];
            out[p] = rec;
        }
        return;
    }
    const double *const part = partials + (size_t)p * kRefineSums * nb;
    if (tid == 0) s_pairs = 0;
    for (int j = 0; j < kNSums; j++) {
        const double v = score_fold(part + (size_t)j * nb, nb, s_w, tid);
        if (tid == 0) s_S[j] = v;
    }
    {
        const unsigned long long *const pc = reinterpret_cast<const unsigned long long *>(part) + (size_t)kNSums * nb;
        unsigned long long mine = 0;
        for (int b = tid; b < nb; b += kBlock) mine += pc[b];
        if (mine) atomicAdd(&s_pairs, mine);
    }
    __syncthreads();
    if (tid != 0) return;
    double S[kNSums];
#pragma unroll
    for (int j = 0; j < kNSums; j++) S[j] = s_S[j];
    const double c[3] = {origin.x, origin.y, origin.z};
    const DeviceSolve rs = solve_rigid_device(static_cast<const double *>(S), c);
    if (rs.degenerate) {
        frozen[p] = 1u;
        for (int k = 0; k < 12; k++) rec.T[k] = T[k];
    } else {
        frozen[p] = 0u;
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = 0; b < 4; b++) {
                double v = (rs.R[3 * a] * T[b] + rs.R[3 * a + 1] * T[4 + b]) + rs.R[3 * a + 2] * T[8 + b];
                if (b == 3) v += rs.t[a];
                rec.T[4 * a + b] = v;
            }
        }
        for (int k = 0; k < 12; k++) T[k] = rec.T[k];
        rec.cost[0] = 0.5 * S[16];
        rec.cost[1] = rs.cost;
        rec.weight_sum = S[0];
        rec.n_pairs = (int64_t)s_pairs;
    }
    out[p] = rec;
}

}  // namespace dev
}  // namespace ppcr
