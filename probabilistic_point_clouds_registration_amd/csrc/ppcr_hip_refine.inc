// Part of the translation unit ppcr_hip.hip: ppcr_scorer_refine — many candidate poses of the scorer's source polished with the
// registration's own objective (radius search with the max_neighbours cut, t / Gaussian weights, the weighted rigid solve),
// all poses in the same launches and no host in between.  Kernels: ppcr_refine.hip.h.

namespace {

constexpr int64_t kRefineMaxPoses = 65535ll * kRefinePosesPerWg;  // (the pose groups are the grid's y dimension)

// the resident target once more, sorted by cells of edge >= radius (the scorer's own grid has ~3 points per cell: right for a
// nearest-neighbour search, wrong for a radius search); from the device copy, rebuilt when the radius changes
int refine_ensure_grid(ppcr_scorer *s)
{
    ppcr_ctx *c = s->c;
    if (s->r_grid_radius == s->r_radius) return PPCR_OK;
    const int nt = (int)c->nt;
    make_grid_desc(nt, c->tgt_lo, c->tgt_hi, s->r_radius, 1, s->r_grid);
    HIP_TRY(c, s->r_tgt.reserve((size_t)nt));
    PPCR_TRY(sort_by_cell(c, s->r_grid, c->tgt_raw.p, nt, s->r_tgt.p, &s->r_cell_start));
    s->r_grid_radius = s->r_radius;
    return PPCR_OK;
}

// a second copy of the source in brick order over cells of its OWN box that hold about four points: 256 consecutive rows
// are one compact region, and stay one under a rigid move.  (score() keeps reading the caller-order copy.)
int refine_ensure_source(ppcr_scorer *s)
{
    ppcr_ctx *c = s->c;
    if (s->r_src_valid) return PPCR_OK;
    const int ns = (int)c->ns;
    PPCR_TRY(bbox_launch(c, c->src.p, ns));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float lo[3], hi[3];
    bbox_fold(c, lo, hi);
    double vol = 1, emax = 0;
    for (int a = 0; a < 3; a++) {
        const double e = (double)hi[a] - (double)lo[a];
        emax = std::max(emax, e);
        vol *= std::max(e, 1e-30);
    }
    double h = std::cbrt(vol * 4.0 / (double)ns);
    if (!(h > emax * 1e-4)) h = std::max(emax * 1e-4, 1e-30);  // flat clouds
    if (!std::isfinite(h) || !(h > 0)) h = 1.0;
    GridDesc g;
    make_grid_desc(ns, lo, hi, h, 1, g);
    HIP_TRY(c, s->r_src.reserve((size_t)ns));
    PPCR_TRY(sort_by_cell(c, g, c->src.p, ns, s->r_src.p, nullptr, 1));
    s->r_src_valid = true;
    return PPCR_OK;
}

Model refine_model(const ppcr_scorer *s)
{
    Model m;
    m.is_normal = !(s->r_dof < std::numeric_limits<double>::infinity());
    m.v = s->r_dof;
    m.texp = -(s->r_dof + s->r_dim) / 2.0;
    m.vpd = s->r_dof + s->r_dim;
    m.vpd_int = 0;
    if (!m.is_normal && m.vpd == std::floor(m.vpd) && m.vpd >= 1 && m.vpd <= 64) m.vpd_int = (int)m.vpd;
    return m;
}

// the search of one iteration: the list width 10 or 20, the model compiled in as K23 has it (t with v + dim = 8, Gaussian,
// or read at run time)
template <int M>
void refine_launch_search(ppcr_scorer *s, const Model &md, dim3 grid, const unsigned *frozen, int np)
{
    ppcr_ctx *c = s->c;
    const float radius = (float)s->r_radius, r2 = (float)(s->r_radius * s->r_radius);
    const double3 origin = make_double3(c->origin[0], c->origin[1], c->origin[2]);
#define PPCR_REFINE_SEARCH(TM)                                                                                                   \
    refine_search_kernel<M, TM><<<grid, kBlock, 0, c->stream>>>(s->r_src.p, (int)c->ns, s->r_poses.p, frozen, np, s->r_tgt.p,    \
                                                                s->r_cell_start.p, s->r_grid, s->box, radius, r2, s->r_max_nb, md, \
                                                                origin, s->r_partials.p)
    if (md.is_normal) PPCR_REFINE_SEARCH(0);
    else if (md.vpd_int == 8) PPCR_REFINE_SEARCH(8);
    else PPCR_REFINE_SEARCH(-1);
#undef PPCR_REFINE_SEARCH
}

}  // namespace

extern "C" {

int ppcr_scorer_set_params(ppcr_scorer *s, double radius, int max_neighbours, double dof, int dim)
{
    if (!s) return PPCR_ERR_INVALID;
    ppcr_ctx *c = s->c;
    CTX_ENTER(c);
    if (!(radius > 0) || !std::isfinite(radius)) return fail(c, PPCR_ERR_INVALID, "radius must be positive and finite");
    if (max_neighbours <= 0 || max_neighbours > 20)
        return fail(c, PPCR_ERR_INVALID, "ppcr_scorer_refine supports 0 < max_neighbours <= 20 (no unbounded search)");
    if (!(dof > 0)) return fail(c, PPCR_ERR_INVALID, "dof must be > 0");
    if (dim <= 0) return fail(c, PPCR_ERR_INVALID, "dim must be > 0");
    s->r_radius = radius;
    s->r_max_nb = max_neighbours;
    s->r_dof = dof;
    s->r_dim = dim;
    s->r_have_params = true;
    return PPCR_OK;
}

int ppcr_scorer_refine(ppcr_scorer *s, const double *T, int64_t n_poses, int n_iter, ppcr_pose_step *last, ppcr_pose_step *history)
{
    if (!s) return PPCR_ERR_INVALID;
    ppcr_ctx *c = s->c;
    CTX_ENTER(c);
    if (n_poses < 0 || n_poses > kRefineMaxPoses) return fail(c, PPCR_ERR_INVALID, "n_poses must be in [0, 262140]");
    if (n_iter < 0) return fail(c, PPCR_ERR_INVALID, "n_iter must be >= 0");
    if (n_poses > 0 && (!T || !last)) return fail(c, PPCR_ERR_INVALID, "null argument");
    if (!c->have_src) return fail(c, PPCR_ERR_STATE, "set a source before ppcr_scorer_refine");
    if (!s->r_have_params) return fail(c, PPCR_ERR_STATE, "ppcr_scorer_set_params before ppcr_scorer_refine");
    s->last_refine_ms = 0;
    if (n_poses == 0) return PPCR_OK;
    const size_t np = (size_t)n_poses;
    if (n_iter == 0 || c->ns == 0) {  // nothing to solve: every record echoes its pose
        for (size_t k = 0; k < np * (size_t)(history ? n_iter + 1 : 1); k++) {
            ppcr_pose_step &r = k < np ? last[k] : history[k - np];
            std::memcpy(r.T, T + 12 * (k % np), sizeof(r.T));
            r.cost[0] = r.cost[1] = r.weight_sum = 0.0;
            r.n_pairs = 0;
        }
        return PPCR_OK;
    }
    PPCR_TRY(ensure_grid(c));  // (the origin of the moments: the centre of the target's box)
    PPCR_TRY(refine_ensure_grid(s));
    PPCR_TRY(refine_ensure_source(s));
    const int nb = nblocks(c->ns);
    const size_t slots = history ? (size_t)n_iter : 1;
    HIP_TRY(c, s->r_partials.reserve(np * (size_t)nb * kRefineSums));
    HIP_TRY(c, s->r_poses.reserve(np * 12));
    HIP_TRY(c, s->r_frozen.reserve(np));
    HIP_TRY(c, s->r_steps.reserve(np * slots));
    for (int k = 0; k < 2; k++)
        if (!s->r_ev[k]) HIP_TRY(c, hipEventCreate(&s->r_ev[k]));
    const Model md = refine_model(s);
    const dim3 grid((unsigned)nb, (unsigned)((n_poses + kRefinePosesPerWg - 1) / kRefinePosesPerWg));
    const double3 origin = make_double3(c->origin[0], c->origin[1], c->origin[2]);

    HIP_TRY(c, hipMemcpyAsync(s->r_poses.p, T, sizeof(double) * 12 * np, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(s->r_ev[0], c->stream));
    for (int it = 0; it < n_iter; it++) {
        // (the first iteration reads no freeze flags and sets them all: nothing to zero)
        const unsigned *frozen = it == 0 ? nullptr : s->r_frozen.p;
        if (s->r_max_nb <= 10) refine_launch_search<10>(s, md, grid, frozen, (int)n_poses);
        else refine_launch_search<20>(s, md, grid, frozen, (int)n_poses);
        PPCR_TRY(check_launch(c, "refine_search_kernel"));
        refine_solve_kernel<<<(unsigned)n_poses, kBlock, 0, c->stream>>>(s->r_partials.p, nb, origin, s->r_poses.p, s->r_frozen.p, it == 0,
                                                                          s->r_steps.p + (history ? (size_t)it * np : 0));
        PPCR_TRY(check_launch(c, "refine_solve_kernel"));
    }
    HIP_TRY(c, hipEventRecord(s->r_ev[1], c->stream));
    ppcr_pose_step *dst = history ? history : last;
    HIP_TRY(c, hipMemcpyAsync(dst, s->r_steps.p, sizeof(ppcr_pose_step) * np * slots, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (history) std::memcpy(last, history + (slots - 1) * np, sizeof(ppcr_pose_step) * np);
    float ms = 0;
    HIP_TRY(c, hipEventElapsedTime(&ms, s->r_ev[0], s->r_ev[1]));
    s->last_refine_ms = ms;
    return PPCR_OK;
}

int ppcr_scorer_last_refine_ms(ppcr_scorer *s, double *ms)
{
    if (!s || !ms) return PPCR_ERR_INVALID;
    *ms = s->last_refine_ms;
    return PPCR_OK;
}

}  // extern "C"
