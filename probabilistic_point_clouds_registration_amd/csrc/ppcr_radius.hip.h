// radius_moments_kernel: the moments of an UNBOUNDED radius search (max_neighbours <= 0: every target inside the radius)
// without an association.  With no cut there is no selection, hence no list to keep: whether a pair belongs is one float
// compare, and its weight needs only the row's normaliser, which is carried along while the candidates stream by (an
// online softmax).  Nothing per pair ever reaches memory; the stored-association route writes a key and a position per
// pair and gathers them again (about 430 M pairs, over 3 GB, per iteration for 1M <-> 1M points at radius 3).
//
// One workgroup per 256 consecutive rows of the (brick-ordered) source, one row per lane:
//   1. the lanes' 27-cell stencils are reduced to the block's range of (y, z) cell rows and x slices; every cell row of
//      that range is ONE contiguous run of the cell-sorted target;
//   2. those runs, laid end to end, stream through an LDS tile of kRadTile points (SoA x / y / z) — a window, not the
//      whole halo, so a row with thousands of neighbours and a row with none take the same code and nothing "does not
//      fit";
//   3. every lane scans the part of the tile that lies in its own nine stencil rows and x windows (the slice clipping
//      of for_each_candidate) and only APPENDS the tile indices of the members to a lane-private LDS list
//      ([slot][lane], 16-bit): about one candidate in six is a member, and f64 weight arithmetic inside the scan would
//      run at a sixth of the lanes;
//   4. the wave drains its lists — slot k for all lanes with k < count, coordinates re-read from the tile — through the
//      f64 pair arithmetic, whenever another sub-chunk could overflow a list and before the tile is overwritten.
// Membership is the exact un-fused float d^2 of every other search here (dist2_flann, strict <) on the unmoved point;
// residuals, weights and moments are f64 at the pose.  That is why there are no matrix instructions in this kernel: MFMA
// has neither the non-FMA float distance nor f64 weights to offer.
// No floating-point atomics: the block's 19 sums are folded in a fixed order (block_reduce_scratch, on the tile's LDS) and
// its pair count, an integer, goes to a slot of its own.
#pragma once
#include "ppcr_device.hip.h"

namespace ppcr {
namespace dev {

constexpr int kRadTile = 2048;      // points per LDS tile (24 KB)
constexpr int kRadSlots = 64;       // list slots per lane (32 KB for the block)
constexpr int kRadSub = 32;         // candidates a lane scans between two looks at the lists' fill
constexpr int kRadRows = kBlock;    // cell rows whose runs are laid end to end at a time (one per thread)
static_assert(kRadTile * 12 >= kFoldScratchBytes, "the block fold borrows the tile");
static_assert(kRadTile <= 65536, "tile indices are 16-bit");

// One row's running sums.  ONEPASS: likelihoods relative to s = 0 (RowMoments as it is).  Otherwise relative to the
// smallest s seen so far: when a smaller one arrives, everything accumulated is rescaled by the likelihood ratio of the
// old minimum to the new one, which reproduces the reference's softmax relative to the row maximum without a second pass.
template <int TM, bool ONEPASS>
struct RadiusRow {
    RowMoments<ONEPASS ? TM : -1> m;  // (two-pass form: storage and finish() only)
    double smin = INFINITY, lp_max = 0;
    __device__ __forceinline__ void begin(const Model &md) { m.begin(md); }
    __device__ __forceinline__ void add_pair(const Model &md, const double (&xr)[3], float yx, float yy, float yz)
    {
        if constexpr (ONEPASS) {
            m.add_pair(md, xr, yx, yy, yz);
        } else {
            const bool normal = TM == 0 || (TM == -1 && md.is_normal);
            const double r0 = (double)yx - xr[0], r1 = (double)yy - xr[1], r2 = (double)yz - xr[2];
            const double sk = fma(r2, r2, fma(r1, r1, r0 * r0));
            if (sk < smin) {
                const double lp_new = TM == -1 ? log_prob(md, sk) : 0.0;  // (only the run-time form reads it)
                if (smin < INFINITY) {
                    const double k = rel_likelihood<TM>(md, smin, sk, lp_new, normal ? 0.0 : fast_rcp(md.v + smin));
                    m.Z *= k, m.G *= k, m.Gs *= k, m.Gr[0] *= k, m.Gr[1] *= k, m.Gr[2] *= k;
                }
                smin = sk, lp_max = lp_new;
            }
            const double inv_vs = normal ? 0.0 : fast_rcp(md.v + sk);
            const double e = rel_likelihood<TM>(md, sk, smin, lp_max, inv_vs);
            const double gk = normal ? e : e * (md.vpd * inv_vs);
            m.Z += e;
            m.G += gk;
            m.Gs = fma(gk, sk, m.Gs);
            m.Gr[0] = fma(gk, r0, m.Gr[0]);
            m.Gr[1] = fma(gk, r1, m.Gr[1]);
            m.Gr[2] = fma(gk, r2, m.Gr[2]);
        }
    }
};

struct RadiusLds {
    float t[3][kRadTile];                      // the tile: x / y / z of kRadTile consecutive points of the stream
    unsigned short list[kRadSlots][kBlock];    // lane-private member lists (tile indices)
    int2 win[9][kBlock];                       // per lane and stencil row: its window [b, e) of the sorted target
    int row_b[kRadRows];                       // per cell row of the batch: where the block's run starts ...
    int row_off[kRadRows + 1];                 // ... and where it starts in the stream (exclusive prefix of the lengths)
    int rng[6];                                // the block's cy / cz / x-slice range
    int wave_sum[kBlock / 64];
    unsigned long long wave_cnt[kBlock / 64];
};

template <int TM, bool ONEPASS>
__global__ __launch_bounds__(kBlock, 2) void radius_moments_kernel(const float4 *__restrict__ src, int ns,
                                                                   const float4 *__restrict__ tgt,
                                                                   const int *__restrict__ cell_start, GridDesc g, float r2,
                                                                   Pose P, Model md, double *__restrict__ partials,
                                                                   unsigned long long *__restrict__ pair_counts)
{
    __shared__ RadiusLds L;
    const int tid = threadIdx.x, nb = gridDim.x;
    const int blk = xcd_block(blockIdx.x, nb);
    const int i = blk * kBlock + tid;
    const bool valid = i < ns;
    const float4 q = valid ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    double xr[3];
    rotated_point(P, q, xr);
    RadiusRow<TM, ONEPASS> row;
    row.begin(md);
    unsigned n_mine = 0;  // members of this lane's row (< nt < 2^31)

    // ---- the lane's stencil, the block's range ----
    const QueryCells qc = query_cells(q, g);
    const int x0 = max(qc.cx - g.xr, 0), x1 = min(qc.cx + g.xr, g.n[0] - 1);
    const bool searching = valid && x0 <= x1;
    if (tid == 0) {
        L.rng[0] = L.rng[2] = L.rng[4] = INT_MAX;
        L.rng[1] = L.rng[3] = L.rng[5] = INT_MIN;
    }
    __syncthreads();
    if (searching) {
        atomicMin(&L.rng[0], qc.cy), atomicMax(&L.rng[1], qc.cy);
        atomicMin(&L.rng[2], qc.cz), atomicMax(&L.rng[3], qc.cz);
        atomicMin(&L.rng[4], x0), atomicMax(&L.rng[5], x1);
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int cy = qc.cy + k % 3 - 1, cz = qc.cz + k / 3 - 1;
        int2 w = make_int2(0, 0);
        if (searching && (unsigned)cy < (unsigned)g.n[1] && (unsigned)cz < (unsigned)g.n[2]) {
            const int base = (cz * g.n[1] + cy) * g.n[0];
            w = make_int2(cell_start[base + x0], cell_start[base + x1 + 1]);
        }
        L.win[k][tid] = w;
    }
    __syncthreads();
    const int ry0 = max(L.rng[0] - 1, 0), ry1 = min(L.rng[1] + 1, g.n[1] - 1);
    const int rz0 = max(L.rng[2] - 1, 0), rz1 = min(L.rng[3] + 1, g.n[2] - 1);
    const int bx0 = L.rng[4], bx1 = L.rng[5];
    const int nyr = ry1 - ry0 + 1;
    // (no lane searches, or every stencil misses the grid: no rows, the loops below do not run)
    const long long n_rows = (L.rng[0] <= L.rng[1] && ry0 <= ry1 && rz0 <= rz1) ? (long long)nyr * (rz1 - rz0 + 1) : 0;

    int cnt = 0;  // entries in this lane's list
    auto drain = [&]() {
        for (int k = 0; __any(k < cnt); k++)
            if (k < cnt) {
                const int idx = L.list[k][tid];
                row.add_pair(md, xr, L.t[0][idx], L.t[1][idx], L.t[2][idx]);
            }
        n_mine += (unsigned)cnt;
        cnt = 0;
    };

    for (long long batch0 = 0; batch0 < n_rows; batch0 += kRadRows) {
        const int rows_here = (int)min((long long)kRadRows, n_rows - batch0);
        // ---- the batch's cell rows: the block's run in each, laid end to end ----
        int run_b = 0, len = 0;
        if (tid < rows_here) {
            const long long r = batch0 + tid;
            const int ry = ry0 + (int)(r % nyr), rz = rz0 + (int)(r / nyr);
            const int base = (rz * g.n[1] + ry) * g.n[0];
            run_b = cell_start[base + bx0];
            len = cell_start[base + bx1 + 1] - run_b;
        }
        int incl = len;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if ((tid & 63) >= d) incl += up;
        }
        __syncthreads();  // (the previous batch's last tile and tables are done with)
        L.row_b[tid] = run_b;
        if ((tid & 63) == 63) L.wave_sum[tid >> 6] = incl;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < (tid >> 6); w++) before += L.wave_sum[w];
        L.row_off[tid] = before + incl - len;
        if (tid == kBlock - 1) L.row_off[kBlock] = before + incl;
        __syncthreads();
        const int stream_len = L.row_off[kBlock];  // (<= nt: the runs are disjoint parts of the target)

        for (int v0 = 0; v0 < stream_len; v0 += kRadTile) {
            const int nv = min(kRadTile, stream_len - v0);
            if (v0 > 0) __syncthreads();  // every wave has drained what it listed from the previous tile
            // ---- stage the tile: stream position -> (row, point) by bisection of the offsets, eight loads in flight ----
            {
                float4 p[kRadTile / kBlock];
#pragma unroll
                for (int u = 0; u < kRadTile / kBlock; u++) {
                    const int v = v0 + min(tid + u * kBlock, nv - 1);
                    int lo = 0, hi = kRadRows;  // row_off[lo] <= v < row_off[hi]
#pragma unroll
                    for (int s = 0; s < 8; s++) {
                        const int mid = (lo + hi) >> 1;
                        if (L.row_off[mid] <= v) lo = mid;
                        else hi = mid;
                    }
                    p[u] = tgt[L.row_b[lo] + (v - L.row_off[lo])];
                }
#pragma unroll
                for (int u = 0; u < kRadTile / kBlock; u++) {
                    const int j = tid + u * kBlock;
                    if (j < nv) L.t[0][j] = p[u].x, L.t[1][j] = p[u].y, L.t[2][j] = p[u].z;
                }
            }
            __syncthreads();
            // ---- scan: the lane's nine windows, clipped to the tile ----
#pragma unroll 1
            for (int k = 0; k < 9; k++) {
                const int2 w = L.win[k][tid];
                int lo = 0, hi = 0;
                if (w.x < w.y) {
                    const long long r = (long long)(qc.cz + k / 3 - 1 - rz0) * nyr + (qc.cy + k % 3 - 1 - ry0) - batch0;
                    if (r >= 0 && r < rows_here) {
                        const int rb = L.row_b[(int)r], rel = L.row_off[(int)r] - v0;  // target position -> tile index
                        lo = max(w.x - rb + rel, 0), hi = min(w.y - rb + rel, nv);
                    }
                }
                while (__any(lo < hi)) {
                    const int end = min(lo + kRadSub, hi);
                    for (; lo < end; lo++) {
                        // dist2_flann: x, y, z in turn, no fused multiply-add
                        const float dx = __fsub_rn(q.x, L.t[0][lo]), dy = __fsub_rn(q.y, L.t[1][lo]), dz = __fsub_rn(q.z, L.t[2][lo]);
                        float d2 = __fmul_rn(dx, dx);
                        d2 = __fadd_rn(d2, __fmul_rn(dy, dy));
                        d2 = __fadd_rn(d2, __fmul_rn(dz, dz));
                        if (d2 < r2) {
                            L.list[cnt][tid] = (unsigned short)lo;
                            cnt++;
                        }
                    }
                    if (__any(cnt > kRadSlots - kRadSub)) drain();
                }
            }
            drain();
        }
    }

    // ---- the block's pair count (integers, fixed order) and its 19 sums ----
    unsigned long long n_wave = n_mine;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_wave += __shfl_down(n_wave, off);
    if ((tid & 63) == 0) L.wave_cnt[tid >> 6] = n_wave;
    RowAcc acc;
#pragma unroll
    for (int j = 0; j < kNSums; j++) acc.a[j] = 0.0;
    if (n_mine > 0) row.m.finish(acc, P, q, xr);  // (rows without a pair contribute nothing, as in accumulate_kernel)
    __syncthreads();  // the tile is free: every wave has drained
    if (tid == 0) pair_counts[blk] = (L.wave_cnt[0] + L.wave_cnt[1]) + (L.wave_cnt[2] + L.wave_cnt[3]);
    double *fold = reinterpret_cast<double *>(&L.t[0][0]);
    block_reduce_scratch(acc, fold, fold + 10 * 257, partials + blk, (size_t)nb, true);
}

// One launch, described by the host code of ppcr_hip_radius.inc and issued by the kernel's own translation unit
// (ppcr_radius.hip, built without packed f32 arithmetic: left to itself the compiler pairs the x and y terms of the
// membership distance into v_pk_add_f32 / v_pk_mul_f32).  tm / onepass: k23_form's choice; tm other than 0 and 8 takes the
// run-time model.
struct RadiusLaunch {
    hipStream_t stream;
    int blocks;
    const float4 *src;
    int ns;
    const float4 *tgt;
    const int *cell_start;
    GridDesc g;
    float r2;
    Pose P;
    Model md;
    int tm;
    bool onepass;
    double *partials;
    unsigned long long *pair_counts;
};
void launch_radius_moments(const RadiusLaunch &a);

}  // namespace dev
}  // namespace ppcr
