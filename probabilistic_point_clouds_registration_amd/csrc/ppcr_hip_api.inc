// Part of the translation unit ppcr_hip.hip: the C ABI of handles, parameters, options, clouds, associations, weights,
// single steps (include/ppcr.h).

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int ppcr_abi_version(void) { return PPCR_ABI_VERSION; }

int ppcr_device_count(int *count)
{
    if (!count) return PPCR_ERR_INVALID;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return PPCR_OK;
}

const char *ppcr_last_error(const ppcr_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int ppcr_create(int device_id, ppcr_ctx **out)
{
    if (!out) return fail(nullptr, PPCR_ERR_INVALID, "out is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, PPCR_ERR_NODEVICE, "no HIP device visible: this library has no CPU fallback");
    }
    if (device_id < 0 || device_id >= n) return fail(nullptr, PPCR_ERR_INVALID, "device_id out of range");
    HIP_TRY(nullptr, hipSetDevice(device_id));
    ppcr_ctx *c = new (std::nothrow) ppcr_ctx();
    if (!c) return fail(nullptr, PPCR_ERR_NOMEM, "out of host memory");
    c->device = device_id;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    // the handle's pinned host memory: ONE device-mapped block (ppcr_pool.hpp: a destroyed handle's block serves the next
    // handle of the device), cut into the mailbox ring, the report ring and the small read-back areas
    auto cut = [](size_t &at, size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) / 256 * 256;
        return here;
    };
    size_t at = 0;
    const size_t o_mbox = cut(at, sizeof(HostMailbox) * kMailboxRing), o_report = cut(at, sizeof(HostReport) * kMailboxRing),
                 o_occ = cut(at, sizeof(unsigned long long) * kOccBins), o_bbox = cut(at, sizeof(float) * 6 * kBboxBlocks),
                 o_sums = cut(at, sizeof(double) * kNSums), o_total = cut(at, sizeof(unsigned long long));
    if (e == hipSuccess) e = pinned_pool(device_id).take(at, reinterpret_cast<void **>(&c->h_pinned));
    char *d_pinned = nullptr;
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&d_pinned), c->h_pinned, 0);
    if (e == hipSuccess) {
        std::memset(c->h_pinned, 0, at);  // (a recycled block: no stale sequence number may look like a result)
        c->h_mbox = reinterpret_cast<HostMailbox *>(c->h_pinned + o_mbox);
        c->d_mbox = reinterpret_cast<HostMailbox *>(d_pinned + o_mbox);
        c->h_report = reinterpret_cast<HostReport *>(c->h_pinned + o_report);
        c->d_report = reinterpret_cast<HostReport *>(d_pinned + o_report);
        c->h_occupancy = reinterpret_cast<unsigned long long *>(c->h_pinned + o_occ);
        c->h_bbox = reinterpret_cast<float *>(c->h_pinned + o_bbox);
        c->h_sums = reinterpret_cast<double *>(c->h_pinned + o_sums);
        c->h_total = reinterpret_cast<unsigned long long *>(c->h_pinned + o_total);
    }
    if (e != hipSuccess) {
        std::string msg = std::string("context setup: ") + hipGetErrorString(e);
        ppcr_destroy(c);
        return fail(nullptr, PPCR_ERR_HIP, msg);
    }
    *out = c;
    return PPCR_OK;
}

int ppcr_destroy(ppcr_ctx *c)
{
    if (!c) return PPCR_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->grid_pending) (void)hipEventSynchronize(c->aux_done);
    if (c->aux_done) (void)hipEventDestroy(c->aux_done);
    for (auto &r : c->prof_recs) {
        (void)hipEventDestroy(r.start);
        (void)hipEventDestroy(r.stop);
    }
    for (auto ev : c->prof_pool) (void)hipEventDestroy(ev);
    release_levels(c);
    c->d_levels.release_idle();
    c->level_inv.release_idle();
    c->level_cap.release_idle();
    c->staging.release_idle();
    c->tgt_raw.release_idle();
    c->tgt_sorted.release_idle();
    c->src.release_idle();
    c->src_alt.release_idle();
    c->cell_start.release_idle();
    c->companion.release_idle();
    c->ground_truth.release_idle();
    c->previous.release_idle();
    c->keys_a.release_idle();
    c->keys_b.release_idle();
    c->vals_a.release_idle();
    c->vals_b.release_idle();
    c->cub_tmp.release_idle();
    c->bbox_part.release_idle();
    c->nbr.release_idle();
    c->dm2.release_idle();
    c->ovf_list.release_idle();
    c->split_flag.release_idle();
    c->split_list.release_idle();
    c->split_state.release_idle();
    c->ovf_state.release_idle();
    c->cnt.release_idle();
    c->row_ptr.release_idle();
    c->gen_counts.release_idle();
    c->gen_row_ptr.release_idle();
    c->gen_pos.release_idle();
    c->gen_keys.release_idle();
    c->d_total.release_idle();
    c->d_stamps.release_idle();
    c->partials.release_idle();
    c->d_sums.release_idle();
    c->d_ticket.release_idle();
    c->d_pose.release_idle();
    c->d_w.release_idle();
    c->d_s.release_idle();
    c->mse_part.release_idle();
    c->d_loop.release_idle();
    c->d_fold_dbg.release_idle();
    c->d_occupancy.release_idle();
    c->d_short.release_idle();
    c->vl.release_idle();
    c->vn.release_idle();
    c->vmask.release_idle();
    c->vstreak.release_idle();
    c->vcount.release_idle();
    c->vorder.release_idle();
    c->vg2.release_idle();
    c->vacc.release_idle();
    c->d_inner_const.release_idle();
    c->d_inner_ctl.release_idle();
    c->track_part.release_idle();
    c->track_ticket.release_idle();
    c->rad_counts.release_idle();
    c->rad_tgt.release_idle();
    c->rad_cell_start.release_idle();
    pinned_pool(c->device).give(c->h_pinned);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return PPCR_OK;
}

#define CTX_ENTER(c)                                  \
    if (!(c)) return PPCR_ERR_INVALID;                \
    HIP_TRY(c, hipSetDevice((c)->device))

int ppcr_set_params(ppcr_ctx *c, double radius, int max_neighbours, double dof, int dim)
{
    CTX_ENTER(c);
    if (!(radius > 0) || !std::isfinite(radius)) return fail(c, PPCR_ERR_INVALID, "radius must be positive and finite");
    if (!(dof > 0)) return fail(c, PPCR_ERR_INVALID, "dof must be > 0 (probabilistic_weights.hpp:34 asserts v > 0)");
    if (dim <= 0) return fail(c, PPCR_ERR_INVALID, "dim must be > 0 (probabilistic_weights.hpp:33)");
    if (radius != c->radius || max_neighbours != c->max_nb) {
        invalidate_association(c);
        c->dm2_valid = false;
    }
    c->radius = radius;
    c->max_nb = max_neighbours;
    c->dof = dof;
    c->dim = dim;
    c->params_set = true;
    return PPCR_OK;
}

int ppcr_set_option(ppcr_ctx *c, const char *key, int value)
{
    CTX_ENTER(c);
    if (!key) return fail(c, PPCR_ERR_INVALID, "null option key");
    PPCR_TRY(grid_settle(c));  // an early grid build was begun under the options as they were: it is dropped
    if (std::strcmp(key, "eager_grid") == 0) {  // ppcr_set_target starts the grid build (on a second stream) when the search is configured
        c->opt_eager_grid = value ? 1 : 0;
        return PPCR_OK;
    }
    if (std::strcmp(key, "sort_source") == 0) {
        if (c->have_src && c->src_sorted && !value)
            return fail(c, PPCR_ERR_STATE, "sort_source can only be switched off before the source has been sorted");
        // (round 5: the x-fastest cell order, value 2, measured slower than the bricks in every configuration, is gone
        //  from the surface, as are "k1_halves" and "mailbox": docs/experiments.md has their numbers)
        if (value != 0 && value != 1) return fail(c, PPCR_ERR_INVALID, "sort_source must be 0 (caller order) or 1 (brick order)");
        c->opt_sort_source = value;  // 0 = keep caller order, 1 = brick/snake order (default)
        return PPCR_OK;
    }
    if (std::strcmp(key, "grid_xf") == 0) {
        if (value != 1 && value != 2 && value != 4 && value != 8) return fail(c, PPCR_ERR_INVALID, "grid_xf must be 1, 2, 4 or 8");
        if (c->have_tgt) return fail(c, PPCR_ERR_STATE, "grid_xf must be set before the target cloud");
        c->opt_grid_xf = value;
        return PPCR_OK;
    }
    if (std::strcmp(key, "brick_x") == 0) {
        if (value != 1 && value != 2 && value != 4) return fail(c, PPCR_ERR_INVALID, "brick_x must be 1, 2 or 4");
        c->opt_brick_xshift = value == 1 ? 0 : (value == 2 ? 1 : 2);
        c->src_sorted = false;
        return PPCR_OK;
    }
    if (std::strcmp(key, "merge_fold") == 0) {
        c->opt_merge_fold = value ? 1 : 0;
        return PPCR_OK;
    }
    if (std::strcmp(key, "fuse_k23") == 0) {
        c->opt_fuse_k23 = value ? 1 : 0;
        return PPCR_OK;
    }
    if (std::strcmp(key, "run_ahead") == 0) {
        c->opt_run_ahead = value ? 1 : 0;
        return PPCR_OK;
    }
    if (std::strcmp(key, "short_lists") == 0) {
        c->opt_short_lists = value ? 1 : 0;
        return PPCR_OK;
    }
    if (std::strcmp(key, "debug_mbox_seq") == 0) {  // TEST HOOK: continue the handle's sequence numbers from `value` (nothing in flight)
        if (value < 0) return fail(c, PPCR_ERR_INVALID, "debug_mbox_seq must be >= 0");
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->mbox_seq = (unsigned)value;
        return PPCR_OK;
    }
    if (std::strcmp(key, "level_stats") == 0) {  // diagnostic: cumulative per-level counters (ppcr_debug_get_levels); setting it clears them
        HIP_TRY(c, c->level_dbg.reserve((size_t)kMaxLevels * kLevelDbgWords));
        HIP_TRY(c, hipMemsetAsync(c->level_dbg.p, 0, (size_t)kMaxLevels * kLevelDbgWords * sizeof(unsigned), c->stream));
        c->opt_level_stats = value ? 1 : 0;
        return PPCR_OK;
    }
    if (std::strcmp(key, "levels") == 0) {
        if (value < -1 || value > 1) return fail(c, PPCR_ERR_INVALID, "levels must be -1 (automatic), 0 (one level) or 1 (same as -1)");
        c->opt_levels = value;
        c->grid_valid = false;
        return PPCR_OK;
    }
    if (std::strcmp(key, "defer_moves") == 0) {
        c->opt_defer_moves = value ? 1 : 0;
        return PPCR_OK;
    }
    if (std::strcmp(key, "two_pass") == 0) {
        if (value < 0 || value > kMaxReach) return fail(c, PPCR_ERR_INVALID, "two_pass must be 0 (off), 1 (automatic) or a reach of 2..8");
        c->opt_two_pass = value;
        c->grid_valid = false;
        return PPCR_OK;
    }
    if (std::strcmp(key, "fuse_max_handed_over") == 0) {
        if (value < 0) return fail(c, PPCR_ERR_INVALID, "fuse_max_handed_over must be >= 0");
        c->opt_fuse_max_handed_over = value;
        return PPCR_OK;
    }
    if (std::strcmp(key, "first_pass_fill") == 0) {
        if (value < 10 || value > 100) return fail(c, PPCR_ERR_INVALID, "first_pass_fill is in tenths of max_neighbours, 10..100");
        c->opt_first_pass_fill = value;
        c->grid_valid = false;
        return PPCR_OK;
    }
    if (std::strcmp(key, "first_pass_occupancy") == 0) {
        if (value < 10 || value > 640) return fail(c, PPCR_ERR_INVALID, "first_pass_occupancy is in tenths of a point per cell, 10..640");
        c->opt_first_pass_occ = value;
        c->grid_valid = false;
        return PPCR_OK;
    }
    if (std::strcmp(key, "fold_stamps") == 0) {
        HIP_TRY(c, c->d_fold_dbg.reserve(8));
        HIP_TRY(c, hipMemsetAsync(c->d_fold_dbg.p, 0, 8 * sizeof(unsigned long long), c->stream));
        c->opt_fold_stamps = value ? 1 : 0;
        return PPCR_OK;
    }
    if (std::strcmp(key, "inner_dev_steps") == 0) {
        if (value < 0 || value > kMaxDevSteps) return fail(c, PPCR_ERR_INVALID, "inner_dev_steps must be in [0, 8]");
        c->opt_inner_dev_steps = value;
        return PPCR_OK;
    }
    if (std::strcmp(key, "verlet") == 0) {  // 1: steady-state associations re-measure Verlet lists instead of searching the grid (default)
        if (value < 0 || value > 2) return fail(c, PPCR_ERR_INVALID, "verlet must be 0 (off), 1 (on) or 2 (diagnostic: lists are built but never trusted)");
        c->opt_verlet = value;
        c->verlet_ok = false;
        c->grid_valid = false;  // (the cells' edge depends on it)
        return PPCR_OK;
    }
    if (std::strcmp(key, "verlet_room") == 0) {
        c->opt_verlet_room = value;
        return PPCR_OK;
    }
    if (std::strcmp(key, "verlet_levels") == 0) {
        c->opt_verlet_levels = value ? 1 : 0;
        c->verlet_ok = false;
        return PPCR_OK;
    }
    if (std::strcmp(key, "verlet_dense") == 0) {
        if (value < 0 || value > 2) return fail(c, PPCR_ERR_INVALID, "verlet_dense must be 0, 1 or 2");
        c->opt_verlet_dense = value;
        c->grid_valid = false;
        return PPCR_OK;
    }
    if (std::strcmp(key, "verlet_engage") == 0) {
        if (value < -1 || value > 100000) return fail(c, PPCR_ERR_INVALID, "verlet_engage is in 1e-4 of the radius, 0 (never) .. 100000 (always); -1: automatic");
        c->opt_verlet_engage = value;
        return PPCR_OK;
    }
    if (std::strcmp(key, "verlet_order") == 0) {
        c->opt_verlet_order = value ? 1 : 0;
        return PPCR_OK;
    }
    if (std::strcmp(key, "verlet_skin") == 0) {
        if (value < 1 || value > 2000) return fail(c, PPCR_ERR_INVALID, "verlet_skin is in 1e-4 of the radius, 1..2000");
        c->opt_verlet_skin = value;
        c->verlet_ok = false;
        c->grid_valid = false;
        return PPCR_OK;
    }
    if (std::strcmp(key, "temporal") == 0) {  // 1: start each query's cut-off from its previous m-th distance (default)
        c->opt_temporal = value ? 1 : 0;
        return PPCR_OK;
    }
    if (std::strcmp(key, "stamps") == 0) {  // diagnostic: per-phase cycle totals of nn_fast_kernel (buffer: see associate_impl)
        c->opt_stamps = value;
        return PPCR_OK;
    }
    return fail(c, PPCR_ERR_INVALID, std::string("unknown option: ") + key);
}

static int set_target_common(ppcr_ctx *c, const void *p, bool dev, int64_t n, int64_t stride)
{
    PPCR_TRY(grid_settle(c));  // (a build of the previous target still reading tgt_raw)
    PPCR_TRY(upload_cloud(c, p, dev, n, stride, c->tgt_raw, true));
    bbox_fold(c, c->tgt_lo, c->tgt_hi);
    c->nt = n;
    c->have_tgt = true;
    c->grid_valid = false;
    c->rad_grid_radius = -1;
    c->origin_valid = false;
    c->dm2_valid = false;
    c->assoc_space = 0;
    invalidate_association(c);
    // (upload_cloud left the main stream idle: nothing earlier still reads the buffers the build writes)
    return grid_begin_early(c);
}

// Sequence numbers (mailbox slots, completion flags, LoopState::finished, the report ring) grow by one per fold for the
// life of a handle and are compared for equality or order; long before the 32-bit counter could wrap — at a new
// source, i.e. between registrations, when nothing is in flight — everything stamped with them starts again from zero.
static int restart_sequence_numbers(ppcr_ctx *c)
{
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->mbox_seq = 0;
    if (c->h_mbox)
        for (int k = 0; k < kMailboxRing; k++) c->h_mbox[k].seq = 0;
    if (c->h_report)
        for (int k = 0; k < kMailboxRing; k++) c->h_report[k].seq = 0;
    if (c->d_inner_ctl.p) HIP_TRY(c, hipMemsetAsync(c->d_inner_ctl.p, 0, c->d_inner_ctl.cap * sizeof(unsigned), c->stream));
    if (c->d_loop.p) HIP_TRY(c, hipMemsetAsync(c->d_loop.p, 0, sizeof(LoopState), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PPCR_OK;
}

static int set_source_common(ppcr_ctx *c, const void *p, bool dev, int64_t n, int64_t stride)
{
    if (c->mbox_seq > (1u << 30)) PPCR_TRY(restart_sequence_numbers(c));
    c->ovf_last = ~0u;
    c->split_clean = false;
    c->level_cap_clean = false;
    c->move_pending = false;  // a deferred move of the previous source dies with it
    c->move_on_device = false;
    c->dm2_valid = false;
    PPCR_TRY(upload_cloud(c, p, dev, n, stride, c->src));
    c->ns = n;
    c->have_src = true;
    // the grid's cells carry the Verlet lists' skin, or not, by an estimate that depends on the source's size (grid_finish):
    // a source for which it comes out the other way has the grid built again (its next use: ensure_grid)
    if (c->grid_valid && c->halo_rho > 0 && !c->opt_verlet_dense) {
        bool big = false;
        if (halo_outgrows_verlet_tile(c, c->halo_rho, c->halo_h, &big) != c->verlet_grid_off) c->grid_valid = false;
        else c->verlet_big_tile = big;  // (same cells either way: only the tile changes)
    }
    c->move_estimate = std::numeric_limits<double>::infinity();  // (a new registration: nothing is known about its moves yet)
    c->move_ratio = std::numeric_limits<double>::quiet_NaN();
    c->move_lag = 1;
    c->pending_from_align = false;
    c->src_sorted = false;
    if (!c->have_companion) c->have_previous = false;  // the snapshot belonged to the previous source
    invalidate_association(c);
    return PPCR_OK;
}

int ppcr_set_target(ppcr_ctx *c, const float *xyz, int64_t n, int64_t stride_bytes)
{
    CTX_ENTER(c);
    return set_target_common(c, xyz, false, n, stride_bytes);
}
int ppcr_set_source(ppcr_ctx *c, const float *xyz, int64_t n, int64_t stride_bytes)
{
    CTX_ENTER(c);
    return set_source_common(c, xyz, false, n, stride_bytes);
}
int ppcr_set_target_device(ppcr_ctx *c, const void *d_xyz, int64_t n, int64_t stride_bytes)
{
    CTX_ENTER(c);
    return set_target_common(c, d_xyz, true, n, stride_bytes);
}
int ppcr_set_source_device(ppcr_ctx *c, const void *d_xyz, int64_t n, int64_t stride_bytes)
{
    CTX_ENTER(c);
    return set_source_common(c, d_xyz, true, n, stride_bytes);
}

int ppcr_associate(ppcr_ctx *c)
{
    CTX_ENTER(c);
    if (!c->have_src || !c->have_tgt) return fail(c, PPCR_ERR_STATE, "set source and target before ppcr_associate");
    return associate_impl(c);
}

int ppcr_association_size(ppcr_ctx *c, int64_t *n_rows, int64_t *nnz)
{
    CTX_ENTER(c);
    PPCR_TRY(ensure_nnz(c));
    if (n_rows) *n_rows = c->ns;
    if (nnz) *nnz = c->nnz;
    return PPCR_OK;
}

int ppcr_get_association(ppcr_ctx *c, int32_t *row_ptr, int32_t *col, float *d2)
{
    CTX_ENTER(c);
    PPCR_TRY(flush_pending_move(c));
    PPCR_TRY(build_csr_cache(c));
    const size_t ns = (size_t)c->ns, nnz = c->h_csr_col.size();
    if (row_ptr) std::memcpy(row_ptr, c->h_csr_row_ptr.data(), sizeof(int) * (ns + 1));
    if (col && nnz) std::memcpy(col, c->h_csr_col.data(), sizeof(int) * nnz);
    if (d2 && nnz) {
        // recomputed from the CURRENT source positions with the kernel's exact float op order
        std::vector<float4> hs(ns), ht((size_t)c->nt);
        HIP_TRY(c, hipMemcpyAsync(hs.data(), c->src.p, sizeof(float4) * ns, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(ht.data(), c->tgt_cur(), sizeof(float4) * (size_t)c->nt, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::vector<float4> so(ns), to((size_t)c->nt);
        for (size_t r = 0; r < ns; r++) { int o; std::memcpy(&o, &hs[r].w, 4); so[(size_t)o] = hs[r]; }
        for (size_t r = 0; r < (size_t)c->nt; r++) { int o; std::memcpy(&o, &ht[r].w, 4); to[(size_t)o] = ht[r]; }
        for (size_t i = 0; i < ns; i++)
            for (int k = c->h_csr_row_ptr[i]; k < c->h_csr_row_ptr[i + 1]; k++) {
                const float4 a = so[i], b = to[(size_t)c->h_csr_col[(size_t)k]];
                volatile float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
                volatile float r = dx * dx;
                volatile float yy = dy * dy;
                r = r + yy;
                volatile float zz = dz * dz;
                r = r + zz;
                d2[k] = r;
            }
    }
    return PPCR_OK;
}

int ppcr_set_association(ppcr_ctx *c, const int32_t *row_ptr, const int32_t *col, int64_t n_rows)
{
    CTX_ENTER(c);
    if (!c->have_src || !c->have_tgt) return fail(c, PPCR_ERR_STATE, "set source and target before ppcr_set_association");
    if (n_rows != c->ns) return fail(c, PPCR_ERR_INVALID, "n_rows must equal the source size");
    if (!row_ptr) return fail(c, PPCR_ERR_INVALID, "null row_ptr");
    const int64_t ns = c->ns;
    if (row_ptr[0] != 0) return fail(c, PPCR_ERR_INVALID, "row_ptr[0] must be 0");
    int maxlen = 0;
    for (int64_t i = 0; i < ns; i++) {
        const int len = row_ptr[i + 1] - row_ptr[i];
        if (len < 0) return fail(c, PPCR_ERR_INVALID, "row_ptr must be non-decreasing");
        maxlen = std::max(maxlen, len);
    }
    const int64_t nnz = row_ptr[ns];
    if (nnz > 0 && !col) return fail(c, PPCR_ERR_INVALID, "null col");
    for (int64_t k = 0; k < nnz; k++)
        if (col[k] < 0 || col[k] >= c->nt) return fail(c, PPCR_ERR_INVALID, "column index out of range");
    invalidate_association(c);
    c->assoc_space = c->grid_valid ? 1 : 0;
    std::vector<int> src_order, tgt_order;
    PPCR_TRY(download_order(c, c->src.p, ns, src_order));
    PPCR_TRY(download_order(c, c->tgt_cur(), c->nt, tgt_order));
    std::vector<int> src_pos((size_t)ns), tgt_pos((size_t)c->nt);
    for (int64_t r = 0; r < ns; r++) src_pos[(size_t)src_order[(size_t)r]] = (int)r;
    for (int64_t r = 0; r < c->nt; r++) tgt_pos[(size_t)tgt_order[(size_t)r]] = (int)r;
    c->h_csr_row_ptr.assign(row_ptr, row_ptr + ns + 1);
    c->h_csr_col.assign(col, col + nnz);
    c->h_csr_slot.resize((size_t)nnz);
    if (maxlen <= kEllMaxWidth) {
        const int w = std::max(maxlen, 1);
        std::vector<int> h_nbr((size_t)w * (size_t)std::max<int64_t>(ns, 1), -1), h_cnt((size_t)std::max<int64_t>(ns, 1), 0);
        for (int64_t i = 0; i < ns; i++) {
            const int r = src_pos[(size_t)i];
            h_cnt[(size_t)r] = row_ptr[i + 1] - row_ptr[i];
            for (int k = row_ptr[i]; k < row_ptr[i + 1]; k++) {
                const size_t sl = (size_t)(k - row_ptr[i]) * (size_t)ns + (size_t)r;
                h_nbr[sl] = tgt_pos[(size_t)col[k]];
                c->h_csr_slot[(size_t)k] = sl;
            }
        }
        HIP_TRY(c, c->nbr.reserve(h_nbr.size()));
        HIP_TRY(c, c->cnt.reserve(h_cnt.size()));
        HIP_TRY(c, hipMemcpyAsync(c->nbr.p, h_nbr.data(), h_nbr.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->cnt.p, h_cnt.data(), h_cnt.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->assoc = ppcr_ctx::ASSOC_ELL;
        c->ell_width = w;
    } else {
        std::vector<int> h_rp((size_t)ns + 1, 0), h_nbr((size_t)std::max<int64_t>(nnz, 1));
        for (int64_t i = 0; i < ns; i++) h_rp[(size_t)src_pos[(size_t)i] + 1] = row_ptr[i + 1] - row_ptr[i];
        for (int64_t r = 0; r < ns; r++) h_rp[(size_t)r + 1] += h_rp[(size_t)r];
        for (int64_t i = 0; i < ns; i++) {
            const int r = src_pos[(size_t)i];
            for (int k = row_ptr[i]; k < row_ptr[i + 1]; k++) {
                const size_t sl = (size_t)h_rp[(size_t)r] + (size_t)(k - row_ptr[i]);
                h_nbr[sl] = tgt_pos[(size_t)col[k]];
                c->h_csr_slot[(size_t)k] = sl;
            }
        }
        HIP_TRY(c, c->row_ptr.reserve(h_rp.size()));
        HIP_TRY(c, c->nbr.reserve(h_nbr.size()));
        HIP_TRY(c, hipMemcpyAsync(c->row_ptr.p, h_rp.data(), h_rp.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->nbr.p, h_nbr.data(), h_nbr.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->assoc = ppcr_ctx::ASSOC_CSR;
    }
    c->nnz = nnz;
    c->csr_cache_valid = true;
    return PPCR_OK;
}

int ppcr_weights(ppcr_ctx *c, const double q[4], const double t[3], double *w_out, double *s_out)
{
    CTX_ENTER(c);
    if (!q || !t) return fail(c, PPCR_ERR_INVALID, "null pose");
    PPCR_TRY(flush_pending_move(c));
    PPCR_TRY(build_csr_cache(c));
    const int ns = (int)c->ns;
    const size_t nnz = c->h_csr_col.size();
    if (nnz == 0) return PPCR_OK;
    const size_t slots = (c->assoc == ppcr_ctx::ASSOC_ELL) ? (size_t)c->ell_width * (size_t)ns : (size_t)c->nnz;
    HIP_TRY(c, c->d_w.reserve(slots));
    HIP_TRY(c, c->d_s.reserve(slots));
    const Mat3 R = quat_to_rot(q);
    const Pose P = make_pose(c, R, t);
    const Model md = make_model(c);
    {
        ProfScope ps(c, K_WEIGHTS);
        if (c->assoc == ppcr_ctx::ASSOC_ELL) {
            EllAssoc a{c->nbr.p, c->cnt.p, ns};
            weights_kernel<EllAssoc><<<nblocks(ns), kBlock, 0, c->stream>>>(a, c->src.p, c->tgt_cur(), ns, P, md, c->d_w.p, c->d_s.p);
        } else {
            CsrAssoc a{c->nbr.p, c->row_ptr.p};
            weights_kernel<CsrAssoc><<<nblocks(ns), kBlock, 0, c->stream>>>(a, c->src.p, c->tgt_cur(), ns, P, md, c->d_w.p, c->d_s.p);
        }
    }
    PPCR_TRY(check_launch(c, "weights_kernel"));
    std::vector<double> hw(slots), hs(slots);
    HIP_TRY(c, hipMemcpyAsync(hw.data(), c->d_w.p, slots * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hs.data(), c->d_s.p, slots * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < nnz; k++) {
        if (w_out) w_out[k] = hw[c->h_csr_slot[k]];
        if (s_out) s_out[k] = hs[c->h_csr_slot[k]];
    }
    return PPCR_OK;
}

int ppcr_accumulate(ppcr_ctx *c, const double q[4], const double t[3], double sums[PPCR_NSUMS])
{
    CTX_ENTER(c);
    if (!q || !t || !sums) return fail(c, PPCR_ERR_INVALID, "null argument");
    return run_accumulate(c, quat_to_rot(q), t, sums);
}

int ppcr_get_origin(ppcr_ctx *c, double o[3])
{
    CTX_ENTER(c);
    if (!o) return fail(c, PPCR_ERR_INVALID, "null argument");
    for (int a = 0; a < 3; a++) o[a] = c->origin_valid ? c->origin[a] : 0.0;
    return PPCR_OK;
}

int ppcr_solve_moments(const double sums[PPCR_NSUMS], const double origin[3], double R[9], double t[3])
{
    if (!sums || !origin || !R || !t) return PPCR_ERR_INVALID;
    const RigidSolve rs = solve_rigid_from_moments(sums, origin);
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) R[3 * a + b] = rs.R.m[a][b];
        t[a] = rs.t[a];
    }
    return rs.degenerate ? 1 : PPCR_OK;
}

double ppcr_cost_from_moments(const double sums[PPCR_NSUMS], const double origin[3], const double R[9], const double t[3])
{
    Mat3 Rm;
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) Rm.m[a][b] = R[3 * a + b];
    return cost_from_moments(sums, origin, Rm, Vec3{{t[0], t[1], t[2]}});
}

int ppcr_update_weights(int device_id, const int32_t *row_ptr, int64_t n_rows, const double *sq_errors, double dof,
                        int dim, double *w_out)
{
    if (!row_ptr || n_rows < 0) return fail(nullptr, PPCR_ERR_INVALID, "bad row_ptr / n_rows");
    if (!(dof > 0) || dim <= 0) return fail(nullptr, PPCR_ERR_INVALID, "dof and dim must be > 0 (probabilistic_weights.hpp:33-34)");
    const int64_t nnz = row_ptr[n_rows];
    if (nnz == 0) return PPCR_OK;
    if (!sq_errors || !w_out) return fail(nullptr, PPCR_ERR_INVALID, "null errors / output");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, PPCR_ERR_NODEVICE, "no HIP device visible: this library has no CPU fallback");
    }
    if (device_id < 0 || device_id >= n) return fail(nullptr, PPCR_ERR_INVALID, "device_id out of range");
    HIP_TRY(nullptr, hipSetDevice(device_id));
    // (scratch from the device's pool: this entry point is ProbabilisticWeights::updateWeights, called once per LM
    //  iteration by user code written against the reference's callback)
    DevBuf<int> rp;
    DevBuf<double> sq, wv;
    auto cleanup = [&]() {
        rp.release();  // (synchronises first: the null stream's kernel and copies are done by then anyway)
        sq.release_idle();
        wv.release_idle();
    };
    hipError_t e = rp.reserve((size_t)(n_rows + 1));
    if (e == hipSuccess) e = sq.reserve((size_t)nnz);
    if (e == hipSuccess) e = wv.reserve((size_t)nnz);
    int *const d_rp = rp.p;
    double *const d_s = sq.p, *const d_w = wv.p;
    if (e == hipSuccess) e = hipMemcpy(d_rp, row_ptr, sizeof(int) * (size_t)(n_rows + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_s, sq_errors, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        ppcr_ctx tmp;  // only used to derive the model constants
        tmp.dof = dof;
        tmp.dim = dim;
        const Model md = make_model(&tmp);
        weights_from_errors_kernel<<<nblocks(n_rows), kBlock>>>(d_rp, n_rows, d_s, md, d_w);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(w_out, d_w, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost);
    cleanup();
    if (e != hipSuccess) return fail(nullptr, PPCR_ERR_HIP, std::string("ppcr_update_weights: ") + hipGetErrorString(e));
    return PPCR_OK;
}

int ppcr_solve(ppcr_ctx *c, const double q0[4], const double t0[3], int max_steps, double f_tol, double T_out[12],
               double cost_out[2], int *steps_out)
{
    CTX_ENTER(c);
    if (!q0 || !t0 || !T_out || !cost_out) return fail(c, PPCR_ERR_INVALID, "null argument");
    return solve_impl(c, q0, t0, max_steps, f_tol, T_out, cost_out, steps_out);
}

int ppcr_apply_transform(ppcr_ctx *c, const double T[12])
{
    CTX_ENTER(c);
    if (!T) return fail(c, PPCR_ERR_INVALID, "null transform");
    return apply_transform_impl(c, T, c->opt_defer_moves != 0);
}

int ppcr_iterate(ppcr_ctx *c, const double q0[4], const double t0[3], int inner_steps, double f_tol, double T_out[12],
                 double cost_out[2], int *steps_out)
{
    CTX_ENTER(c);
    if (!q0 || !t0 || !T_out || !cost_out) return fail(c, PPCR_ERR_INVALID, "null argument");
    if (!c->have_src || !c->have_tgt) return fail(c, PPCR_ERR_STATE, "set source and target before ppcr_iterate");
    {
        const double qn = q0[0] * q0[0] + q0[1] * q0[1] + q0[2] * q0[2] + q0[3] * q0[3];
        if (!(qn > 0) || !std::isfinite(qn)) return fail(c, PPCR_ERR_INVALID, "initial rotation quaternion has zero or non-finite norm");
    }
    PPCR_TRY(associate_impl(c));
    PPCR_TRY(solve_impl(c, q0, t0, inner_steps, f_tol, T_out, cost_out, steps_out));
    return apply_transform_impl(c, T_out, /*defer=*/true);
}

int ppcr_stop_rule_check(ppcr_stop_rule *rule, int n_iter, double cost_drop_thresh, double n_cost_drop_it)
{
    if (!rule) return PPCR_ERR_INVALID;
    if (rule->iteration == n_iter) return PPCR_STOP_MAX_ITERATIONS;  // cc:140
    if (!(rule->cost_drop < cost_drop_thresh)) {                     // also taken by a NaN drop (cc:154-156)
        rule->idle = 0;
        return PPCR_CONTINUE;
    }
    if ((double)rule->idle > n_cost_drop_it) return PPCR_STOP_COST_DROP;  // cc:146
    rule->idle += 1;
    return PPCR_CONTINUE;
}

}  // extern "C"
