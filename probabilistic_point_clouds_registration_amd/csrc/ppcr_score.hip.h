// Scoring many candidate poses of one source against one resident target (ppcr_scorer, include/ppcr.h): the kernels.
//
// Per chunk of poses, all on one stream and with no host round trip in between:
//   score_search_kernel    d2[p][i] = exact nearest-target d^2 of float(T_p x_i), + first-digit histogram + f64 partial sums
//   score_resolve_kernel   histogram + rank -> digit of the wanted order statistic, remaining rank (one workgroup per pose)
//   score_digit_hist_kernel  histogram of the next digit among the elements that match the prefix found so far
//   score_band_kernel      count below the band, count and f64 partial sums inside it
//   score_finish_kernel    partials folded in block order -> ppcr_pose_score[p]
// An order statistic is found by radix select on the float pattern (d^2 >= 0: the pattern orders like an unsigned), digits of
// 11 / 11 / 10 bits from the top; up to two ranks per pose (the reference's even-n "median" averages two elements).
//
// Everything a score depends on is either an integer count (atomics allowed) or an f64 sum folded in a fixed order, so two
// calls with the same inputs return the same bits.  d^2 itself is a minimum: no scan order can change it.
//
// The kernels are compiled without packed-f32 instructions (PPCR_SCORE_KERNEL).
#pragma once
#include "ppcr.h"
#include "ppcr_device.hip.h"

namespace ppcr {
namespace dev {

#if defined(__HIP_DEVICE_COMPILE__)
#define PPCR_SCORE_KERNEL __attribute__((target("no-packed-fp32-ops")))
#else
#define PPCR_SCORE_KERNEL
#endif

constexpr int kScorePosesPerWg = 4;    // poses a workgroup of the search takes, its 256 queries held in registers
constexpr int kScoreBins = 2048;       // bins of the widest digit
constexpr int kScoreItems = 16;        // elements per lane of the streaming passes (4096 per workgroup)
constexpr int kScoreSpan = kBlock * kScoreItems;

// the bounding box of the finite target coordinates (exact: a float min / max)
struct ScoreBox {
    float lo[3], hi[3];
};

// per pose: the (up to two) order statistics a selection round is looking for
struct ScoreSel {
    unsigned prefix[2];  // the digits found so far, right-aligned
    unsigned rank[2];    // rank among the elements that match the prefix
    unsigned active[2];
    unsigned count;      // elements the round selects from (decides odd / even)
    unsigned pad;
};

// what the later kernels need of a chunk, in one struct (device pointers into the scorer's scratch)
struct ScoreScratch {
    float *d2;                // [poses][nq]
    unsigned *hist1;          // [poses][2048]: top 11 bits, written by the search
    unsigned *hist2[2];       // per round: [poses][2][2048]
    unsigned *hist3[2];       // per round: [poses][2][1024]
    double *psum;             // [poses][search blocks]
    unsigned *band_below;     // [poses][stream blocks]
    unsigned *band_in;        // [poses][stream blocks]
    double *band_sum;         // [poses][stream blocks]
    ScoreSel *sel;            // [poses]
    double *median;           // [2][poses]: the round's result
    unsigned long long *robust_count;  // [poses]
};

// rigid move of one point, the arithmetic of move_point / transform_kernel: f64, summed left to right, f32 store
__device__ __forceinline__ void score_move(const float4 q, const double *__restrict__ T, float out[3])
{
    const double x = q.x, y = q.y, z = q.z;
    out[0] = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
    out[1] = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
    out[2] = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
}

// One query's view of the grid: its clamped cell, the cell edges, and how far it lies outside the target's box per axis.
struct ScoreQuery {
    float qp[3];
    int c0[3];
    float out2[3];  // (distance to the box on this axis, less eps, not below 0)^2
};

__device__ __forceinline__ void score_query_setup(ScoreQuery &s, const GridDesc &g, const ScoreBox &box)
{
    const float inv[3] = {g.inv_hx, g.inv_h, g.inv_h};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        s.c0[a] = clampi(cell_coord(s.qp[a], g.org[a], inv[a], g.n[a]), 0, g.n[a] - 1);
        const float o = fmaxf(fmaxf(box.lo[a] - s.qp[a], s.qp[a] - box.hi[a]) - g.eps, 0.f);
        s.out2[a] = o * o;
    }
}

// Lower bound on the squared distance from the query to every target NOT in the block [lo, hi] of cells.  Such a target lies
// beyond a face of the block that is not a face of the grid, and inside the target's box on the other two axes: at least
// gap_face on the face's axis (nn1_kernel's bound, same eps) and at least the query's distance to the box on the others.  For
// a query far outside the box the lateral term is what lets the search stop after a few shells: the scanned block only has to
// reach sqrt(2 D delta), not D.  0: no bound (a face within eps of the query).
__device__ __forceinline__ float score_bound2(const ScoreQuery &s, const GridDesc &g, const float edge[3], const int lo[3],
                                              const int hi[3])
{
    float b2 = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float f = s.qp[a] - g.org[a];
        const float lateral = s.out2[(a + 1) % 3] + s.out2[(a + 2) % 3];
        if (lo[a] > 0) {
            const float gap = f - (float)lo[a] * edge[a] - g.eps;
            b2 = fminf(b2, gap > 0.f ? gap * gap + lateral : 0.f);
        }
        if (hi[a] < g.n[a] - 1) {
            const float gap = (float)(hi[a] + 1) * edge[a] - f - g.eps;
            b2 = fminf(b2, gap > 0.f ? gap * gap + lateral : 0.f);
        }
    }
    return b2;
}

__device__ __forceinline__ float score_wave_min(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ double score_wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ int score_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float score_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// One query searched by a whole wave, from shell rho0 on, until the bound holds.  `best` is the minimum over what the lane that
// owns the query has already scanned (shells below rho0).  Every (y, z) row of a shell is one contiguous run of the
// cell-sorted target: rows of the two z faces are dealt to the wave's four 16-lane groups, the two y-face rows of every other
// plane take 32 lanes each, and the rows inside (two end cells each) go one per lane.  Returns the wave-wide minimum.
__device__ __forceinline__ float score_wave_search(const ScoreQuery &s, float best, int rho0, const GridDesc &g,
                                                   const float4 *__restrict__ tgt, const int *__restrict__ cell_start, int lane)
{
    const float edge[3] = {g.h / (float)g.xr, g.h, g.h};
    const float4 q = make_float4(s.qp[0], s.qp[1], s.qp[2], 0.f);
    auto scan = [&](int b, int e, int first, int step) {
        for (int p = b + first; p < e; p += step) best = fminf(best, dist2_flann(q, tgt[p]));
    };
    for (int rho = rho0;; rho++) {
        int lo[3], hi[3];
        bool whole = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            lo[a] = max(s.c0[a] - rho, 0);
            hi[a] = min(s.c0[a] + rho, g.n[a] - 1);
            whole = whole && lo[a] == 0 && hi[a] == g.n[a] - 1;
        }
        for (int z = lo[2]; z <= hi[2]; z++) {
            if (z == s.c0[2] - rho || z == s.c0[2] + rho) {
                for (int y = lo[1] + (lane >> 4); y <= hi[1]; y += 4) {
                    const int base = (z * g.n[1] + y) * g.n[0];
                    scan(cell_start[base + lo[0]], cell_start[base + hi[0] + 1], lane & 15, 16);
                }
            } else {
                const int y = lane < 32 ? s.c0[1] - rho : s.c0[1] + rho;
                if (y >= 0 && y <= g.n[1] - 1) {
                    const int base = (z * g.n[1] + y) * g.n[0];
                    scan(cell_start[base + lo[0]], cell_start[base + hi[0] + 1], lane & 31, 32);
                }
            }
        }
        // rows that touch the shell only with their two end cells
        const int iy0 = max(s.c0[1] - rho + 1, 0), iy1 = min(s.c0[1] + rho - 1, g.n[1] - 1);
        const int iz0 = max(s.c0[2] - rho + 1, 0), iz1 = min(s.c0[2] + rho - 1, g.n[2] - 1);
        const int niy = iy1 - iy0 + 1, niz = iz1 - iz0 + 1;
        if (niy > 0 && niz > 0) {
            const int xa = s.c0[0] - rho, xb = s.c0[0] + rho;
            for (int r = lane; r < niy * niz; r += 64) {
                const int base = ((iz0 + r / niy) * g.n[1] + iy0 + r % niy) * g.n[0];
                if (xa >= 0) scan(cell_start[base + xa], cell_start[base + xa + 1], 0, 1);
                if (xb <= g.n[0] - 1) scan(cell_start[base + xb], cell_start[base + xb + 1], 0, 1);
            }
        }
        best = score_wave_min(best);
        if (whole) break;
        const float b2 = score_bound2(s, g, edge, lo, hi);
        if (b2 > 0.f && best <= b2 * 0.999999f) break;
    }
    return best;
}

// ---------------------------------------------------------------------------------------------------------------------------
// 1. The search.  Grid: (blocks of 256 queries) x (groups of kScorePosesPerWg poses).  Per pose every lane moves its query and
// scans shells 0 and 1 of its clamped cell by itself (nn1_kernel's scan); with ~3 targets per cell that answers nearly every
// query that lies in the target.  Lanes still open — and lanes more than two cells outside the box, which skip the private
// scan: it could not answer them — are compacted into a list in LDS and searched one per wave (score_wave_search).
// ---------------------------------------------------------------------------------------------------------------------------
PPCR_SCORE_KERNEL __global__ __launch_bounds__(kBlock) void score_search_kernel(
    const float4 *__restrict__ queries, int nq, const double *__restrict__ poses, int n_poses, const float4 *__restrict__ tgt,
    const int *__restrict__ cell_start, GridDesc g, ScoreBox box, float *__restrict__ d2_out, unsigned *__restrict__ hist1,
    double *__restrict__ psum)
{
    __shared__ unsigned s_hist[kScoreBins];
    __shared__ float s_q[kBlock][3];
    __shared__ float s_best[kBlock];
    __shared__ int s_list[kBlock];  // lane | first shell to scan << 16
    __shared__ int s_count;
    __shared__ double s_wsum[kBlock / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * kBlock + tid;
    const bool valid = i < nq;
    const float4 q0 = valid ? queries[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = tid; b < kScoreBins; b += kBlock) s_hist[b] = 0;
    const float edge[3] = {g.h / (float)g.xr, g.h, g.h};
    const float far2 = 4.f * g.h * g.h;

    const int p_begin = blockIdx.y * kScorePosesPerWg, p_end = min(p_begin + kScorePosesPerWg, n_poses);
    for (int p = p_begin; p < p_end; p++) {
        if (tid == 0) s_count = 0;
        __syncthreads();
        ScoreQuery s;
        score_move(q0, poses + (size_t)p * 12, s.qp);
        score_query_setup(s, g, box);
        const float4 q = make_float4(s.qp[0], s.qp[1], s.qp[2], 0.f);
        float best = INFINITY;
        bool done = !valid;
        int rho_next = 0;
        if (valid && !(s.out2[0] + s.out2[1] + s.out2[2] > far2)) {
            for (int rho = 0; rho < 2 && !done; rho++) {
                int lo[3], hi[3];
                bool whole = true;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    lo[a] = max(s.c0[a] - rho, 0);
                    hi[a] = min(s.c0[a] + rho, g.n[a] - 1);
                    whole = whole && lo[a] == 0 && hi[a] == g.n[a] - 1;
                }
                for (int z = lo[2]; z <= hi[2]; z++)
                    for (int y = lo[1]; y <= hi[1]; y++) {
                        const int base = (z * g.n[1] + y) * g.n[0];
                        // (rho <= 1: every row of the block is a shell row except the centre row of shell 1)
                        if (rho == 0 || y != s.c0[1] || z != s.c0[2]) {
                            const int b = cell_start[base + lo[0]], e = cell_start[base + hi[0] + 1];
                            for (int t = b; t < e; t++) best = fminf(best, dist2_flann(q, tgt[t]));
                        } else {
                            if (s.c0[0] - 1 >= 0) {
                                const int b = cell_start[base + s.c0[0] - 1], e = cell_start[base + s.c0[0]];
                                for (int t = b; t < e; t++) best = fminf(best, dist2_flann(q, tgt[t]));
                            }
                            if (s.c0[0] + 1 <= g.n[0] - 1) {
                                const int b = cell_start[base + s.c0[0] + 1], e = cell_start[base + s.c0[0] + 2];
                                for (int t = b; t < e; t++) best = fminf(best, dist2_flann(q, tgt[t]));
                            }
                        }
                    }
                rho_next = rho + 1;
                if (whole) {
                    done = true;
                } else {
                    const float b2 = score_bound2(s, g, edge, lo, hi);
                    done = b2 > 0.f && best <= b2 * 0.999999f;
                }
            }
        }
        // the open lanes, compacted: one LDS counter bump per wave
        {
            const unsigned long long open = __ballot(!done);
            int slot0 = 0;
            if (lane == 0 && open) slot0 = atomicAdd(&s_count, __popcll(open));
            slot0 = __shfl(slot0, 0, 64);
            if (!done) {
                const int slot = slot0 + __builtin_amdgcn_mbcnt_hi((unsigned)(open >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)open, 0));
                s_list[slot] = tid | (rho_next << 16);
                s_q[tid][0] = s.qp[0];
                s_q[tid][1] = s.qp[1];
                s_q[tid][2] = s.qp[2];
                s_best[tid] = best;
            }
        }
        __syncthreads();
        {
            const int count = s_count;
            for (int k = wave; k < count; k += kBlock / 64) {
                const int entry = score_uniform(s_list[k]);
                const int owner = entry & 0xFFFF;
                ScoreQuery w;
#pragma unroll
                for (int a = 0; a < 3; a++) w.qp[a] = score_uniform(s_q[owner][a]);
                score_query_setup(w, g, box);
                const float r = score_wave_search(w, score_uniform(s_best[owner]), entry >> 16, g, tgt, cell_start, lane);
                if (lane == 0) s_best[owner] = r;
            }
        }
        __syncthreads();
        if (valid && !done) best = s_best[tid];

        // d2, the first digit's histogram (non-zero bins only reach global memory) and the block's f64 partial sum
        const unsigned bin = __float_as_uint(best) >> 21;
        if (valid) {
            d2_out[(size_t)p * (size_t)nq + (size_t)i] = best;
            atomicAdd(&s_hist[bin], 1u);
        }
        const double ws = score_wave_sum(valid ? (double)best : 0.0);
        if (lane == 0) s_wsum[wave] = ws;
        __syncthreads();
        if (valid) {
            const unsigned v = atomicExch(&s_hist[bin], 0u);  // exactly one lane per bin gets the count and leaves the bin empty
            if (v) atomicAdd(&hist1[(size_t)p * kScoreBins + bin], v);
        }
        if (tid == 0) {
            double t = s_wsum[0];
            for (int k = 1; k < kBlock / 64; k++) t += s_wsum[k];
            psum[(size_t)p * gridDim.x + blockIdx.x] = t;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// 2. Radix select.  score_resolve_kernel: one workgroup per pose turns (histogram of a digit, rank) into (that digit, rank
// among the elements that share it).  `init` starts a round: 1 the median's ranks from n, 2 the robust median's ranks from the
// band pass — below + index, the in-band values being a contiguous range of the sorted order.  `last` ends it: the prefix is
// then the whole float pattern, and the round's result (the reference's index rule, see ppcr.h) goes to median_out.
// ---------------------------------------------------------------------------------------------------------------------------
PPCR_SCORE_KERNEL __global__ __launch_bounds__(kBlock) void score_resolve_kernel(
    ScoreSel *__restrict__ sel, const unsigned *__restrict__ hist, int bins_log2, int per_slot, int init, int last, unsigned n,
    const unsigned *__restrict__ band_below, const unsigned *__restrict__ band_in, int stream_blocks,
    unsigned long long *__restrict__ robust_count, double *__restrict__ median_out)
{
    __shared__ ScoreSel s;
    __shared__ unsigned s_part[kBlock];
    __shared__ unsigned s_below, s_in;
    const int p = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        s_below = 0;
        s_in = 0;
        if (!init) s = sel[p];
    }
    __syncthreads();
    if (init == 2) {
        unsigned below = 0, in = 0;
        for (int b = tid; b < stream_blocks; b += kBlock) {
            below += band_below[(size_t)p * stream_blocks + b];
            in += band_in[(size_t)p * stream_blocks + b];
        }
        if (below) atomicAdd(&s_below, below);
        if (in) atomicAdd(&s_in, in);
        __syncthreads();
    }
    if (init && tid == 0) {
        const unsigned m = init == 1 ? n : s_in, below = init == 1 ? 0u : s_below;
        if (init == 2) robust_count[p] = m;
        s.count = m;
        s.prefix[0] = s.prefix[1] = 0;
        // sorted[(m + 1) / 2] for odd m, the mean of sorted[m / 2] and sorted[m / 2 + 1] for even m; fewer than 3: none
        s.active[0] = m >= 3;
        s.active[1] = m >= 3 && m % 2 == 0;
        s.rank[0] = below + (m % 2 ? (m + 1) / 2 : m / 2);
        s.rank[1] = below + m / 2 + 1;
    }
    __syncthreads();
    const int bins = 1 << bins_log2, per = bins / kBlock;
    for (int k = 0; k < 2; k++) {
        if (!s.active[k]) continue;  // (uniform)
        const unsigned *h = hist + ((size_t)p * (per_slot ? 2 : 1) + (per_slot ? k : 0)) * bins;
        unsigned mine = 0;
        for (int b = 0; b < per; b++) mine += h[tid * per + b];
        s_part[tid] = mine;
        __syncthreads();
        unsigned before = 0;
        for (int t = 0; t < tid; t++) before += s_part[t];
        const unsigned rank = s.rank[k];
        __syncthreads();
        if (rank >= before && rank < before + mine) {  // exactly one lane: rank < the number of elements under the prefix
            unsigned acc = before;
            for (int b = 0; b < per; b++) {
                const unsigned c = h[tid * per + b];
                if (rank < acc + c) {
                    s.prefix[k] = (s.prefix[k] << bins_log2) | (unsigned)(tid * per + b);
                    s.rank[k] = rank - acc;
                    break;
                }
                acc += c;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        sel[p] = s;
        if (last) {
            double r = __longlong_as_double(0x7FF8000000000000ll);
            if (s.active[0]) {
                r = (double)__uint_as_float(s.prefix[0]);
                if (s.active[1]) r = (r + (double)__uint_as_float(s.prefix[1])) / 2.0;
            }
            median_out[p] = r;
        }
    }
}

// histogram of the digit at `shift` (`bins_log2` bits) among the elements whose bits above it equal the slot's prefix
PPCR_SCORE_KERNEL __global__ __launch_bounds__(kBlock) void score_digit_hist_kernel(const float *__restrict__ d2, int nq,
                                                                                     const ScoreSel *__restrict__ sel,
                                                                                     unsigned *__restrict__ hist, int shift,
                                                                                     int bins_log2)
{
    __shared__ unsigned s_hist[2 * kScoreBins];
    const int p = blockIdx.y, tid = threadIdx.x;
    const ScoreSel s = sel[p];
    if (!s.active[0] && !s.active[1]) return;  // (uniform)
    const int bins = 1 << bins_log2;
    for (int b = tid; b < 2 * bins; b += kBlock) s_hist[b] = 0;
    __syncthreads();
    const float *row = d2 + (size_t)p * (size_t)nq;
    const int above = shift + bins_log2;  // (< 32: the first digit is the search's)
    for (int k = 0; k < kScoreItems; k++) {
        const int64_t i = (int64_t)blockIdx.x * kScoreSpan + k * kBlock + tid;
        if (i >= nq) break;
        const unsigned bits = __float_as_uint(row[i]);
        const unsigned digit = (bits >> shift) & (unsigned)(bins - 1);
        if (s.active[0] && (bits >> above) == s.prefix[0]) atomicAdd(&s_hist[digit], 1u);
        if (s.active[1] && (bits >> above) == s.prefix[1]) atomicAdd(&s_hist[bins + digit], 1u);
    }
    __syncthreads();
    for (int b = tid; b < 2 * bins; b += kBlock) {
        const unsigned v = s_hist[b];
        if (v) atomicAdd(&hist[(size_t)p * 2 * bins + b], v);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// 3. The band  median / factor <= v <= median * factor, evaluated in double as the reference does: per block the count below
// it, the count inside it and the f64 sum of what is inside (lane-serial, then a fixed tree).  A NaN median leaves all three 0.
// ---------------------------------------------------------------------------------------------------------------------------
PPCR_SCORE_KERNEL __global__ __launch_bounds__(kBlock) void score_band_kernel(const float *__restrict__ d2, int nq,
                                                                               const double *__restrict__ median, double factor,
                                                                               unsigned *__restrict__ band_below,
                                                                               unsigned *__restrict__ band_in,
                                                                               double *__restrict__ band_sum)
{
    __shared__ unsigned s_below[kBlock / 64], s_in[kBlock / 64];
    __shared__ double s_sum[kBlock / 64];
    const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double med = median[p], hi = med * factor, lo = med / factor;
    const float *row = d2 + (size_t)p * (size_t)nq;
    unsigned below = 0, in = 0;
    double sum = 0.0;
    for (int k = 0; k < kScoreItems; k++) {
        const int64_t i = (int64_t)blockIdx.x * kScoreSpan + k * kBlock + tid;
        if (i >= nq) break;
        const double v = (double)row[i];
        if (v <= hi && v >= lo) {
            in++;
            sum += v;
        } else if (v < lo) {
            below++;
        }
    }
    sum = score_wave_sum(sum);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        below += __shfl_xor(below, m, 64);
        in += __shfl_xor(in, m, 64);
    }
    if (lane == 0) {
        s_below[wave] = below;
        s_in[wave] = in;
        s_sum[wave] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kBlock / 64; k++) {
            below += s_below[k];
            in += s_in[k];
            sum += s_sum[k];
        }
        const size_t at = (size_t)p * gridDim.x + blockIdx.x;
        band_below[at] = below;
        band_in[at] = in;
        band_sum[at] = sum;
    }
}

// in block order: lane t adds partials t, t + 256, ... in turn, then the fixed tree
__device__ __forceinline__ double score_fold(const double *__restrict__ part, int n, double *s_w, int tid)
{
    double v = 0.0;
    for (int b = tid; b < n; b += kBlock) v += part[b];
    v = score_wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) s_w[tid >> 6] = v;
    __syncthreads();
    v = s_w[0];
    for (int k = 1; k < kBlock / 64; k++) v += s_w[k];
    return v;
}

// 4. One workgroup per pose: the partial sums folded, the score written.
PPCR_SCORE_KERNEL __global__ __launch_bounds__(kBlock) void score_finish_kernel(const double *__restrict__ psum, int search_blocks,
                                                                                 const double *__restrict__ band_sum,
                                                                                 int stream_blocks,
                                                                                 const double *__restrict__ median, int n_poses,
                                                                                 const unsigned long long *__restrict__ robust_count,
                                                                                 ppcr_pose_score *__restrict__ out)
{
    __shared__ double s_w[kBlock / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    const double sum = score_fold(psum + (size_t)p * search_blocks, search_blocks, s_w, tid);
    const double rsum = score_fold(band_sum + (size_t)p * stream_blocks, stream_blocks, s_w, tid);
    if (tid == 0) {
        ppcr_pose_score r;
        r.sum = sum;
        r.median = median[p];
        r.robust_sum = rsum;
        r.robust_count = (int64_t)robust_count[p];
        r.robust_median = median[(size_t)n_poses + p];
        out[p] = r;
    }
}

}  // namespace dev
}  // namespace ppcr
