// Batches of small cloud pairs with a cell-grid search (ppcr_batch_run_small_grid, include/ppcr.h): the kernel.  One workgroup
// of 256 lanes registers one pair, as small_align_kernel (ppcr_small.hip.h) does and with its loop, its solve lane
// (small_solve_lane below), its stopping rule and its records; what differs is the search.  small_align_kernel measures every target
// point from every source row in every outer iteration; here the workgroup sorts the target into a uniform grid of its own,
// once, and a row looks at the 27 cells around it.
//
//   small_grid_align_kernel<M, TM>   grid: one workgroup per pair; M, TM as small_align_kernel has them.
//
// Geometry (host, small_grid_geometry in ppcr_hip_small_grid.inc): origin = the low corner of the target's box, cell edge
// h = 1.001 r + 16 eps max|coord| (never below the radius, the eps term covers the float rounding of a cell
// coordinate), enlarged until nx ny nz <= kSmallGridCells.  A cell coordinate is floor((v - org) * inv_h), one float subtract
// and one float multiply, for targets and rows alike; the host counts the cells with the same expression, so every finite
// target lies in [0, n) and two points closer than the radius lie at most one cell apart on every axis.
//
// The sort (small_grid_sort), used twice per pair before the first iteration — the target never moves, and the source is
// sorted by the TARGET's cells at its initial position, keys clamped into the grid, only so that a wave's rows stay
// neighbours and share cache lines:
//   histogram   one LDS atomic per point on a table of 16-bit counts, two to a 32-bit word (a count is at most 16384: no carry);
//   scan        every lane sums its own words, a wave scan, the four wave totals through LDS: exclusive cell starts;
//   scatter     STABLE, by wave-level multi-split.  The points go through in chunks of 256 in index order.  A lane finds the
//               lanes of its wave with its key (one ballot per key bit), its rank = the peers below it, and the lowest peer
//               advances the cell's cursor by the peer count with one LDS atomic; the four waves take that turn one after
//               the other, a barrier between them.  A cell's points therefore lie in ascending original index whatever the
//               hardware does, and the sorted arrays are a function of the input alone.  The cost is 4 barriers and <= 13
//               ballots per 256 points for ANY distribution: all points in one cell is one atomic per wave and chunk, the
//               cheapest case, not the worst.  (The other route, atomics and then ordering each cell's run, sorts 16384
//               entries of one cell in that case.)
// After the target's scatter a cursor has reached its cell's end: table[c] = start of cell c + 1, and start(c) = table[c - 1].
// The sorted target is float4 {x, y, z, original index bits} in per-pair device scratch (16 nt bytes: 256 KB at 16384 points,
// it does not fit LDS next to the lists and the fold), the sorted source xyz behind it (12 ns bytes), moved in place.  Both
// are written and read by this workgroup only, a barrier in between.
//
// The search of a row: its cell, each axis clamped to [-2, n + 1] (NaN: -2); the stencil clipped to the grid.  A surviving
// (dy, dz) row of cells is ONE run of the sorted target, nine at most, walked four candidates at a time (the loads of a
// group are in flight together; a group none of which beats the current limit costs one comparison) and offered to the
// lane's list with refine_offer / refine_select: the (d^2, original index) order, the strict d^2 < float(r r) and the ties of
// every other search of the library.  A row two or more cells outside the grid on some axis has an empty stencil.  A
// non-finite target point is binned by its clamped key and fails every distance test, a non-finite row has no stencil:
// neither pairs with anything, as in small_align_kernel.  A list entry is a POSITION in the sorted target (16 bits), and so
// are the winners stored for the later inner steps.
//
// LDS: table 16 KB + lists 16 KB + the fold's 21.3 KB + the solve lane's state: 54 KB, two workgroups per CU.
// Deviations from the plan of the issue: a target with an infinite coordinate gets ONE cell with inv_h = 0 (every row scans
// every target: exact) instead of a box over its finite points; the sorted target is never staged into LDS (not measured).
// Every loop is bounded by a launch argument or a descriptor field (runs are clamped to nt): no flags, no global atomics,
// no waiting on anybody.  A pair's bits depend on that pair alone.
#pragma once
#include "ppcr_small.hip.h"

namespace ppcr {
namespace dev {

constexpr int kSmallGridCells = 8192;  // cells of a pair's grid at most: the LDS table, 16-bit entries
constexpr int kSmallGridKeyBits = 13;
static_assert((1 << kSmallGridKeyBits) >= kSmallGridCells, "the multi-split compares this many key bits");
static_assert(PPCR_SMALL_MAX_POINTS < 0x8000, "two 16-bit cursors share a word: no carry from the low one");

struct SmallGridPair {
    SmallPair p;                     // (nbr_off: the pair's winners, sorted positions, in u16)
    unsigned long long scratch_off;  // bytes, a multiple of 16: float4 sorted target [nt], then xyz sorted source [ns]
    float org[3], inv_h;
    int n[3];
};

struct SmallGridArgs {
    SmallArgs a;  // (a.pairs unused)
    const SmallGridPair *pairs;
    unsigned char *scratch;
};

// cell coordinate on one axis, clamped to [-2, n + 1]; NaN -> -2
__device__ __forceinline__ int small_grid_cell(float v, float org, float inv_h, int n)
{
    const float f = floorf((v - org) * inv_h);
    return (int)fminf(fmaxf(f, -2.0f), (float)(n + 1));
}
// the cell of a point, clamped into the grid, x fastest
__device__ __forceinline__ int small_grid_key(const float *p, const SmallGridPair &g)
{
    const int cx = clampi(small_grid_cell(p[0], g.org[0], g.inv_h, g.n[0]), 0, g.n[0] - 1);
    const int cy = clampi(small_grid_cell(p[1], g.org[1], g.inv_h, g.n[1]), 0, g.n[1] - 1);
    const int cz = clampi(small_grid_cell(p[2], g.org[2], g.inv_h, g.n[2]), 0, g.n[2] - 1);
    return (cz * g.n[1] + cy) * g.n[0] + cx;
}
// entry c of the table of 16-bit values
__device__ __forceinline__ int small_grid_entry(const unsigned *tab, int c) { return (int)((tab[c >> 1] >> ((c & 1) * 16)) & 0xFFFFu); }

// Points 0 .. n - 1 with key_of(i) in [0, ncells) to their places in cell order, stable: emit(i, position).  Leaves
// tab[c] = the end of cell c.  Called by the whole workgroup; s_wave: kBlock / 64 words.
template <class KeyOf, class Emit>
__device__ __forceinline__ void small_grid_sort(int n, int ncells, unsigned *tab, int *s_wave, KeyOf key_of, Emit emit)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nwords = (ncells + 1) / 2;
    __syncthreads();  // nobody reads the table that was there
    for (int w = tid; w < nwords; w += kBlock) tab[w] = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += kBlock) {
        const int k = key_of(i);
        atomicAdd(&tab[k >> 1], 1u << ((k & 1) * 16));
    }
    __syncthreads();
    {  // counts -> exclusive starts: a lane owns whole words
        const int per = (nwords + kBlock - 1) / kBlock, w0 = min(tid * per, nwords), w1 = min(w0 + per, nwords);
        int sum = 0;
        for (int w = w0; w < w1; w++) sum += (int)(tab[w] & 0xFFFFu) + (int)(tab[w] >> 16);
        int inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        int run = inc - sum;
        for (int w = 0; w < wave; w++) run += s_wave[w];
        for (int w = w0; w < w1; w++) {
            const unsigned v = tab[w], first = (unsigned)run, second = first + (v & 0xFFFFu);
            tab[w] = first | (second << 16);
            run = (int)(second + (v >> 16));
        }
    }
    __syncthreads();
    int nbits = 0;
    while ((1 << nbits) < ncells) nbits++;  // (<= kSmallGridKeyBits)
    for (int base = 0; base < n; base += kBlock) {  // (uniform)
        const int i = base + tid;
        const bool valid = i < n;
        const int k = valid ? key_of(i) : 0;
        unsigned long long peers = __ballot(valid);
        for (int b = 0; b < nbits; b++) {
            const bool bit = (k >> b) & 1;
            const unsigned long long v = __ballot(bit);
            peers &= bit ? v : ~v;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull)), count = __popcll(peers);
        const int shift = (k & 1) * 16;
        unsigned old = 0u;
        for (int w = 0; w < kBlock / 64; w++) {  // the waves in turn: chunk order is index order
            if (w == wave && valid && rank == 0) old = atomicAdd(&tab[k >> 1], (unsigned)count << shift);
            __syncthreads();
        }
        old = __shfl(old, valid ? __ffsll((long long)peers) - 1 : lane, 64);  // from the lowest peer
        if (valid) emit(i, (int)((old >> shift) & 0xFFFFu) + rank);
    }
    __syncthreads();
}

// The solve lane's turn once a step's moments are folded into s_S: the rigid solve, the inner loop's test, and either the
// pose of the next inner step (s_go = 1) or the end of the outer iteration — T_cum <- T_step T_cum, the records, the
// source's pending move, the stopping rule (s_go = 2: the next iteration, 0: stop).  The pointers are the kernel's LDS
// variables.  This is the block small_align_kernel has inline, statement for statement; calling this function from there
// was tried and changes that kernel's compiled code, which has to stay as it is.
__device__ __forceinline__ void small_solve_lane(const SmallArgs &a, const double (&c)[3], size_t pair, int it, int step,
                                                 const double *s_S, double *s_pose, double *s_move, double *s_Tcum,
                                                 SmallRule &s_rule, double &s_cost_init, int &s_go)
{
    double Sm[kNSums];
#pragma unroll
    for (int j = 0; j < kNSums; j++) Sm[j] = s_S[j];
    const DeviceSolve rs = solve_rigid_device(static_cast<const double *>(Sm), c);
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
        return;
    }
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

// the sorted target and a lane's list of positions in it
struct SmallGridCands {
    const float4 *tgt;
    unsigned short *list;  // [slot * kBlock + tid]
    int tid;
    __device__ __forceinline__ float4 get(int e) const { return tgt[e]; }
    __device__ __forceinline__ unsigned orig_of(int e) const { return __float_as_uint(tgt[e].w); }
    __device__ __forceinline__ int load(int t) const { return list[t * kBlock + tid]; }
    __device__ __forceinline__ void store(int t, int e) const { list[t * kBlock + tid] = (unsigned short)e; }
};

template <int M, int TM>
PPCR_SCORE_KERNEL __global__ __launch_bounds__(kBlock) void small_grid_align_kernel(SmallGridArgs ga)
{
    __shared__ unsigned s_cells[kSmallGridCells / 2];
    __shared__ unsigned short s_list[kRefineList * kBlock];
    __shared__ int s_wave[kBlock / 64];
    __shared__ double s_S[kNSums];
    __shared__ double s_pose[12];  // as in small_align_kernel, these seven
    __shared__ double s_move[12];
    __shared__ double s_Tcum[12];
    __shared__ SmallRule s_rule;
    __shared__ double s_cost_init;
    __shared__ int s_go;

    const int tid = threadIdx.x;
    const SmallArgs &a = ga.a;
    const SmallGridPair g = ga.pairs[blockIdx.x];
    const size_t pair = (size_t)a.first + blockIdx.x;
    const int ns = g.p.ns, nt = g.p.nt, m = a.m;
    float4 *const tgt = reinterpret_cast<float4 *>(ga.scratch + g.scratch_off);
    float *const src = reinterpret_cast<float *>(tgt + nt);
    unsigned short *const nbr = a.nbr != nullptr ? a.nbr + g.p.nbr_off : nullptr;
    const int nchunks = (ns + kBlock - 1) / kBlock;
    const int n0 = g.n[0], n1 = g.n[1], n2 = g.n[2];
    const unsigned r2_bits = __float_as_uint(a.r2);

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
    {  // the source, then the target (whose table stays); the sort's barriers also publish the solve lane's state
        const float *const psrc = a.packed + g.p.src_off, *const ptgt = a.packed + g.p.tgt_off;
        small_grid_sort(ns, n0 * n1 * n2, s_cells, s_wave, [&](int i) { return small_grid_key(psrc + 3 * (size_t)i, g); },
                        [&](int i, int pos) {
                            const float *const p = psrc + 3 * (size_t)i;
                            src[3 * (size_t)pos] = p[0], src[3 * (size_t)pos + 1] = p[1], src[3 * (size_t)pos + 2] = p[2];
                        });
        small_grid_sort(nt, n0 * n1 * n2, s_cells, s_wave, [&](int i) { return small_grid_key(ptgt + 3 * (size_t)i, g); },
                        [&](int i, int pos) {
                            const float *const p = ptgt + 3 * (size_t)i;
                            tgt[pos] = make_float4(p[0], p[1], p[2], __int_as_float(i));
                        });
    }
    const SmallGridCands S{tgt, s_list, tid};

    for (int it = 0; it < a.n_iter; it++) {
        if (s_go == 0) break;  // (uniform: written before the last barrier)
        for (int step = 1; step <= a.inner_steps; step++) {
            Pose P;  // the step's pose, about the pair's origin
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int k = 0; k < 3; k++) P.R[3 * r + k] = s_pose[4 * r + k];
                P.t[r] = s_pose[4 * r + 3];
                P.c[r] = g.p.c[r];
            }
            RowAcc acc;
#pragma unroll
            for (int j = 0; j < kNSums; j++) acc.a[j] = 0.0;

            for (int ch = 0; ch < nchunks; ch++) {
                const int i = ch * kBlock + tid;
                const bool valid = i < ns;
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
                if (valid) q = make_float4(src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], 0.f);
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
                    if (valid) {
                        unsigned lim = r2_bits;
                        const int cx = small_grid_cell(q.x, g.org[0], g.inv_h, n0), cy = small_grid_cell(q.y, g.org[1], g.inv_h, n1),
                                  cz = small_grid_cell(q.z, g.org[2], g.inv_h, n2);
                        const int x0 = max(cx - 1, 0), x1 = min(cx + 1, n0 - 1);
                        for (int dz = -1; dz <= 1 && x0 <= x1; dz++) {
                            if ((unsigned)(cz + dz) >= (unsigned)n2) continue;
                            for (int dy = -1; dy <= 1; dy++) {
                                if ((unsigned)(cy + dy) >= (unsigned)n1) continue;
                                const int row = ((cz + dz) * n1 + (cy + dy)) * n0;
                                const int b = row + x0 > 0 ? small_grid_entry(s_cells, row + x0 - 1) : 0;
                                const int e = min(small_grid_entry(s_cells, row + x1), nt);
                                for (int p = b; p < e; p += 4) {
                                    unsigned d[4];
#pragma unroll
                                    for (int u = 0; u < 4; u++) {
                                        const float4 t = tgt[min(p + u, e - 1)];
                                        d[u] = p + u < e ? __float_as_uint(dist2_flann(q, t)) : 0xFFFFFFFFu;
                                    }
                                    if (min(min(d[0], d[1]), min(d[2], d[3])) < lim) {
#pragma unroll
                                        for (int u = 0; u < 4; u++) refine_offer<M>(S, q, p + u, d[u], n, lim, m);
                                    }
                                }
                            }
                        }
                        if (n > m) {
                            unsigned T;
                            n = refine_select<M>(S, q, n, m, T);
                        }
                        if (nbr != nullptr)
                            for (int j = 0; j < m; j++) nbr[(size_t)j * ns + i] = j < n ? (unsigned short)S.load(j) : kSmallNone;
                    }
                } else if (valid) {  // a later step: the stored winners, in the order they were stored in
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
            if (tid == 0) small_solve_lane(a, g.p.c, pair, it, step, s_S, s_pose, s_move, s_Tcum, s_rule, s_cost_init, s_go);
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
