// Part of the translation unit ppcr_hip.hip: iterations on the implicit association of an unbounded radius search
// (max_neighbours <= 0).  radius_moments_kernel (ppcr_radius.hip.h) leaves the partial moments of that association at a
// pose without ever storing a pair; the fold, the solve and the mailbox are the ones every other step uses.  The loop is
// host-paced on purpose: a step is hundreds of microseconds to milliseconds of kernel, one mailbox round trip is noise.

namespace {

struct RadiusGrid {  // the cell-sorted target the kernel streams: cells of edge >= radius, one cell of reach
    const float4 *tgt;
    const int *cell_start;
    GridDesc g;
};

// What a call needs before its first launch.  The handle's own grid serves when it is a one-pass grid of the current
// radius (every unbounded search's is: grid_begin sizes the cells by the radius unless the search is bounded).  A handle
// with no association to disturb gets its grid and its source order made current as ppcr_associate would; otherwise the
// grid logic is left alone and a second, radius-sized grid of the target is kept beside it.
int radius_prepare(ppcr_ctx *c, RadiusGrid &rg)
{
    if (!c->have_tgt || !c->have_src) return fail(c, PPCR_ERR_STATE, "set source and target before a radius iteration");
    if (!c->params_set) return fail(c, PPCR_ERR_STATE, "ppcr_set_params before a radius iteration");
    PPCR_TRY(flush_pending_move(c));
    std::memset(&rg, 0, sizeof(rg));
    if (c->ns == 0 || c->nt == 0) return PPCR_OK;  // (nothing is searched: launch_radius_step runs no row)
    if (c->assoc == ppcr_ctx::ASSOC_NONE) {
        PPCR_TRY(ensure_grid(c));
        PPCR_TRY(ensure_source_sorted(c));
    }
    if (c->grid_valid && c->grid_radius == c->radius && c->grid_max_nb == c->max_nb && c->reach == 1) {
        rg.tgt = c->tgt_sorted.p, rg.cell_start = c->cell_start.p, rg.g = c->grid;
        return PPCR_OK;
    }
    if (c->rad_grid_radius != c->radius) {
        PPCR_TRY(grid_settle(c));  // (an early build of the handle's grid shares the sort scratch)
        const int nt = (int)c->nt;
        make_grid_desc(nt, c->tgt_lo, c->tgt_hi, c->radius, c->opt_grid_xf, c->rad_grid);
        HIP_TRY(c, c->rad_tgt.reserve((size_t)nt));
        PPCR_TRY(sort_by_cell(c, c->rad_grid, c->tgt_raw.p, nt, c->rad_tgt.p, &c->rad_cell_start));
        c->rad_grid_radius = c->radius;
    }
    rg.tgt = c->rad_tgt.p, rg.cell_start = c->rad_cell_start.p, rg.g = c->rad_grid;
    return PPCR_OK;
}

int radius_blocks(const ppcr_ctx *c) { return (c->ns > 0 && c->nt > 0) ? nblocks(c->ns) : 1; }

// enqueue the kernel at the pose (R, t), then the fold and the solve; nothing here waits for the device
int launch_radius_step(ppcr_ctx *c, const RadiusGrid &rg, const Mat3 &R, const double t[3], StepTicket &tk)
{
    if (!c->origin_valid) c->origin[0] = c->origin[1] = c->origin[2] = 0;  // (no grid of the handle's own: as launch_step)
    const int ns = (c->ns > 0 && c->nt > 0) ? (int)c->ns : 0;  // an empty cloud: one workgroup, no row, zero moments
    const int nb = radius_blocks(c);
    const float r2 = (float)(c->radius * c->radius);  // PCL: static_cast<float>(radius * radius)
    const Pose P = make_pose(c, R, t);
    const Model md = make_model(c);
    HIP_TRY(c, c->partials.reserve((size_t)nb * kNSums));
    HIP_TRY(c, c->rad_counts.reserve((size_t)nb));
    {
        ProfScope ps(c, K_RADIUS);
        // the models compiled in are K23's (k23_form); an integer v + dim other than 8 takes the run-time form
        const K23Form f = k23_form(c, md);
        launch_radius_moments(RadiusLaunch{c->stream, nb, c->src.p, ns, rg.tgt, rg.cell_start, rg.g, r2, P, md, f.tm, f.onepass,
                                           c->partials.p, c->rad_counts.p});
    }
    PPCR_TRY(check_launch(c, "radius_moments_kernel"));
    FoldSolve fs;
    PPCR_TRY(prepare_fold(c, nb, tk, fs, nullptr));
    {
        ProfScope ps(c, K_REDUCE);
        reduce_solve_kernel<<<kNSums, kBlock, 0, c->stream>>>(fs);
    }
    return check_launch(c, "reduce_solve_kernel");
}

// the pair count of the last step: the blocks' integer counts, added in block order (membership does not depend on the pose)
int radius_pair_count(ppcr_ctx *c, int64_t *n_pairs)
{
    std::vector<unsigned long long> per_block((size_t)radius_blocks(c));
    HIP_TRY(c, hipMemcpyAsync(per_block.data(), c->rad_counts.p, per_block.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned long long total = 0;
    for (unsigned long long v : per_block) total += v;
    *n_pairs = (int64_t)total;
    return PPCR_OK;
}

int iterate_radius_impl(ppcr_ctx *c, const double q0[4], const double t0[3], int inner_steps, double f_tol, double T_out[12],
                        double cost_out[2], int *steps_out, int64_t *n_pairs)
{
    RadiusGrid rg;
    PPCR_TRY(radius_prepare(c, rg));
    PPCR_TRY(irls_loop(c, q0, t0, inner_steps, f_tol, T_out, cost_out, steps_out,
                       [c, &rg](const Mat3 &R, const double t[3], StepTicket &tk) { return launch_radius_step(c, rg, R, t, tk); }));
    if (n_pairs) PPCR_TRY(radius_pair_count(c, n_pairs));
    return apply_transform_impl(c, T_out);
}

}  // namespace

extern "C" {

int ppcr_accumulate_radius(ppcr_ctx *c, const double q[4], const double t[3], double sums[PPCR_NSUMS], int64_t *n_pairs)
{
    CTX_ENTER(c);
    if (!q || !t || !sums) return fail(c, PPCR_ERR_INVALID, "null argument");
    RadiusGrid rg;
    PPCR_TRY(radius_prepare(c, rg));
    StepTicket tk;
    StepResult res;
    PPCR_TRY(launch_radius_step(c, rg, quat_to_rot(q), t, tk));
    PPCR_TRY(collect_step(c, tk, res));
    std::memcpy(sums, res.sums, sizeof(res.sums));
    if (n_pairs) PPCR_TRY(radius_pair_count(c, n_pairs));
    return PPCR_OK;
}

int ppcr_iterate_radius(ppcr_ctx *c, const double q0[4], const double t0[3], int inner_steps, double f_tol, double T_out[12],
                        double cost_out[2], int *steps_out, int64_t *n_pairs)
{
    CTX_ENTER(c);
    if (!q0 || !t0 || !T_out || !cost_out) return fail(c, PPCR_ERR_INVALID, "null argument");
    return iterate_radius_impl(c, q0, t0, inner_steps, f_tol, T_out, cost_out, steps_out, n_pairs);
}

int ppcr_align_radius(ppcr_ctx *c, int n_iter, double cost_drop_thresh, double n_cost_drop_it, const double q0[4],
                      const double t0[3], int inner_steps, double f_tol, double *history, double *costs, int32_t *steps,
                      int *n_done)
{
    CTX_ENTER(c);
    if (!q0 || !t0) return fail(c, PPCR_ERR_INVALID, "null argument");
    if (n_iter < 0 && (history || costs || steps))
        return fail(c, PPCR_ERR_INVALID, "ppcr_align_radius: n_iter < 0 (no iteration cap) needs history, costs and steps to be NULL");
    if (n_iter < 0 && !(cost_drop_thresh > 0))
        return fail(c, PPCR_ERR_INVALID, "ppcr_align_radius: n_iter < 0 (no iteration cap) needs cost_drop_thresh > 0, or the loop never ends");
    ppcr_stop_rule rule{};
    double Tcum[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    while (ppcr_stop_rule_check(&rule, n_iter, cost_drop_thresh, n_cost_drop_it) == PPCR_CONTINUE) {
        double Tk[12], cost[2];
        int st = 0;
        PPCR_TRY(iterate_radius_impl(c, q0, t0, inner_steps, f_tol, Tk, cost, &st, nullptr));
        compose(Tk, Tcum, Tcum);  // T_cum <- T_k * T_cum
        const int it = rule.iteration;
        if (history) std::memcpy(history + (size_t)it * 12, Tcum, sizeof(Tcum));
        if (costs) costs[2 * it] = cost[0], costs[2 * it + 1] = cost[1];
        if (steps) steps[it] = st;
        rule.cost_drop = (cost[0] - cost[1]) / cost[0];
        rule.iteration++;
    }
    if (n_done) *n_done = rule.iteration;
    return PPCR_OK;
}

}  // extern "C"
