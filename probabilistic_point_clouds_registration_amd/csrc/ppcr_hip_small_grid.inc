// Part of the translation unit ppcr_hip.hip: ppcr_batch_run_small_grid — ppcr_batch_run_small with a cell-grid search that
// every workgroup builds for its own pair.  The host side is small_batch_run (ppcr_hip_small.inc: validation, packing, the
// launch cut, the records); this file adds what the grid needs: a pair's geometry, its device scratch and the launch.
// Kernel: ppcr_small_grid.hip.h.

namespace {

// The grid of one pair from its target's box [lo, hi] (what the packing loop found) and the radius: origin, 1 / cell edge,
// cells per axis.  h = 1.001 r + 16 eps max|coord|, then larger by a tenth at a time until the cells fit the kernel's table.
// The cells of an axis are counted with the kernel's own float expression (small_grid_cell), so that the target's last
// point lies in cell n - 1 exactly.  A box that is not finite (an empty or all-NaN target, an infinite coordinate, an
// extent beyond float) gets one cell and inv_h = 0: every finite row then lands in that cell.
void small_grid_geometry(const float lo[3], const float hi[3], double radius, SmallGridPair &d)
{
    d.n[0] = d.n[1] = d.n[2] = 1;
    d.org[0] = d.org[1] = d.org[2] = 0.f;
    d.inv_h = 0.f;
    float ext[3], maxc = 0.f;
    for (int x = 0; x < 3; x++) {
        ext[x] = hi[x] - lo[x];
        if (!std::isfinite(lo[x]) || !std::isfinite(hi[x]) || !std::isfinite(ext[x])) return;
        maxc = std::max(maxc, std::max(std::fabs(lo[x]), std::fabs(hi[x])));
    }
    double h = 1.001 * radius + 16.0 * (double)FLT_EPSILON * (double)maxc;
    for (int tries = 0; tries < 4096; tries++, h *= 1.1) {
        const float inv_h = 1.0f / (float)h;  // (h beyond float: 0, one cell)
        long long cells = 1;
        int n[3];
        for (int x = 0; x < 3; x++) {
            n[x] = (int)std::min(std::floor(ext[x] * inv_h), (float)kSmallGridCells) + 1;
            cells *= n[x];
        }
        if (cells > kSmallGridCells) continue;
        for (int x = 0; x < 3; x++) d.n[x] = n[x], d.org[x] = lo[x];
        d.inv_h = inv_h;
        return;
    }
}

template <int M>
void small_grid_launch(const SmallGridArgs &g, unsigned n, hipStream_t stream)
{
    if (g.a.md.is_normal) small_grid_align_kernel<M, 0><<<n, kBlock, 0, stream>>>(g);
    else if (g.a.md.vpd_int == 8) small_grid_align_kernel<M, 8><<<n, kBlock, 0, stream>>>(g);
    else small_grid_align_kernel<M, -1><<<n, kBlock, 0, stream>>>(g);
}

struct SmallGrid {
    typedef SmallGridPair Desc;
    static constexpr const char *name = "ppcr_batch_run_small_grid", *kernel = "small_grid_align_kernel";
    static SmallPair &base(Desc &d) { return d.p; }
    // the sorted target as float4 and the sorted source as xyz
    static size_t scratch_bytes(int64_t ns, int64_t nt) { return 16 * (size_t)nt + 12 * (size_t)ns; }
    static void describe(Desc &d, const float *lo, const float *hi, double radius, size_t scratch_at)
    {
        d.scratch_off = scratch_at;
        small_grid_geometry(lo, hi, radius, d);
    }
    static void launch(SmallArgs &a, const Desc *pairs, void *scratch, unsigned n, hipStream_t stream)
    {
        const SmallGridArgs g{a, pairs, static_cast<unsigned char *>(scratch)};
        if (a.m <= 10) small_grid_launch<10>(g, n, stream);
        else small_grid_launch<20>(g, n, stream);
    }
};

}  // namespace

extern "C" {

int ppcr_batch_run_small_grid(const ppcr_pair *pairs, int64_t n_pairs, const ppcr_batch_options *opt, int device_id, double *T_all,
                              int32_t *n_iter_done, double *history, double *costs, int32_t *steps, char *err, int64_t err_capacity)
{
    return small_batch_run<SmallGrid>(pairs, n_pairs, opt, device_id, T_all, n_iter_done, history, costs, steps, err, err_capacity);
}

}  // extern "C"
