// Part of the translation unit ppcr_hip.hip: ppcr_scorer — many candidate poses of one source scored against one resident
// target in one call (the closest-point metrics of utilities.hpp:28-234 as a swarm's fitness function).  Kernels:
// ppcr_score.hip.h.

#ifndef PPCR_SCORE_D2_BYTES
#define PPCR_SCORE_D2_BYTES (256ll << 20)  // d2 scratch of one chunk of poses
#endif

struct ppcr_scorer {
    ppcr_ctx *c = nullptr;  // private handle: the target, its grid, the source (caller order), the stream
    ScoreBox box{};
    DevBuf<double> d_poses, d_f64;           // d_f64: psum | band_sum | median[2]
    DevBuf<float> d_d2;
    DevBuf<unsigned> d_u32;                  // hist1 | hist2[2] | hist3[2] | band_below | band_in  (the histograms zeroed per chunk)
    DevBuf<ScoreSel> d_sel;
    DevBuf<unsigned long long> d_rcount;
    DevBuf<ppcr_pose_score> d_scores;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> search_events;  // one pair per chunk of the last call
    size_t search_events_used = 0;
    double last_search_ms = 0;
    // ppcr_scorer_refine (ppcr_hip_refine.inc): its parameters, the target sorted by cells of edge >= radius, the source in
    // brick order of its own box, and the scratch of a call
    bool r_have_params = false, r_src_valid = false;
    double r_radius = 0, r_dof = 0, r_grid_radius = -1;
    int r_max_nb = 0, r_dim = 3;
    GridDesc r_grid{};
    DevBuf<float4> r_tgt, r_src;
    DevBuf<int> r_cell_start;
    DevBuf<double> r_partials, r_poses;  // r_partials: [pose][kRefineSums][blocks]
    DevBuf<unsigned> r_frozen;
    DevBuf<ppcr_pose_step> r_steps;
    hipEvent_t r_ev[2] = {nullptr, nullptr};
    double last_refine_ms = 0;
};

namespace {

// everything one chunk of `np` poses enqueues; scores of the chunk land in s->d_scores
int score_chunk(ppcr_scorer *s, const double *T, int np, int cap, double factor, size_t chunk_index)
{
    ppcr_ctx *c = s->c;
    const int nq = (int)c->ns;
    const int search_blocks = nblocks(nq), stream_blocks = nblocks(nq, kScoreSpan);
    // the scratch, cut for `cap` poses (the same cut for every chunk of a call)
    ScoreScratch w;
    w.d2 = s->d_d2.p;
    unsigned *u = s->d_u32.p;
    w.hist1 = u, u += (size_t)cap * kScoreBins;
    for (int r = 0; r < 2; r++) w.hist2[r] = u, u += (size_t)cap * 2 * kScoreBins;
    for (int r = 0; r < 2; r++) w.hist3[r] = u, u += (size_t)cap * 2 * (kScoreBins / 2);
    const size_t hist_words = (size_t)(u - s->d_u32.p);
    w.band_below = u, u += (size_t)cap * stream_blocks;
    w.band_in = u;
    double *d = s->d_f64.p;
    w.psum = d, d += (size_t)cap * search_blocks;
    w.band_sum = d, d += (size_t)cap * stream_blocks;
    w.median = d;
    w.sel = s->d_sel.p;
    w.robust_count = s->d_rcount.p;

    HIP_TRY(c, hipMemcpyAsync(s->d_poses.p, T, sizeof(double) * 12 * (size_t)np, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(s->d_u32.p, 0, hist_words * sizeof(unsigned), c->stream));
    if (s->search_events.size() <= chunk_index) {
        std::pair<hipEvent_t, hipEvent_t> ev;
        HIP_TRY(c, hipEventCreate(&ev.first));
        HIP_TRY(c, hipEventCreate(&ev.second));
        s->search_events.push_back(ev);
    }
    HIP_TRY(c, hipEventRecord(s->search_events[chunk_index].first, c->stream));
    score_search_kernel<<<dim3(search_blocks, (np + kScorePosesPerWg - 1) / kScorePosesPerWg), kBlock, 0, c->stream>>>(
        c->src.p, nq, s->d_poses.p, np, c->tgt_sorted.p, c->cell_start.p, c->grid, s->box, w.d2, w.hist1, w.psum);
    PPCR_TRY(check_launch(c, "score_search_kernel"));
    HIP_TRY(c, hipEventRecord(s->search_events[chunk_index].second, c->stream));
    s->search_events_used = chunk_index + 1;

    // two selection rounds: the median, then (behind the band pass) the robust median
    for (int round = 0; round < 2; round++) {
        if (round == 1) {
            score_band_kernel<<<dim3(stream_blocks, np), kBlock, 0, c->stream>>>(w.d2, nq, w.median, factor, w.band_below, w.band_in,
                                                                                 w.band_sum);
            PPCR_TRY(check_launch(c, "score_band_kernel"));
        }
        double *med = w.median + (size_t)round * cap;
        score_resolve_kernel<<<np, kBlock, 0, c->stream>>>(w.sel, w.hist1, 11, 0, round + 1, 0, (unsigned)nq, w.band_below, w.band_in,
                                                           stream_blocks, w.robust_count, med);
        score_digit_hist_kernel<<<dim3(stream_blocks, np), kBlock, 0, c->stream>>>(w.d2, nq, w.sel, w.hist2[round], 10, 11);
        score_resolve_kernel<<<np, kBlock, 0, c->stream>>>(w.sel, w.hist2[round], 11, 1, 0, 0, (unsigned)nq, w.band_below, w.band_in,
                                                           stream_blocks, w.robust_count, med);
        score_digit_hist_kernel<<<dim3(stream_blocks, np), kBlock, 0, c->stream>>>(w.d2, nq, w.sel, w.hist3[round], 0, 10);
        score_resolve_kernel<<<np, kBlock, 0, c->stream>>>(w.sel, w.hist3[round], 10, 1, 0, 1, (unsigned)nq, w.band_below, w.band_in,
                                                           stream_blocks, w.robust_count, med);
        PPCR_TRY(check_launch(c, "score selection"));
    }
    score_finish_kernel<<<np, kBlock, 0, c->stream>>>(w.psum, search_blocks, w.band_sum, stream_blocks, w.median, cap, w.robust_count,
                                                      s->d_scores.p);
    return check_launch(c, "score_finish_kernel");
}

}  // namespace

extern "C" {

int ppcr_scorer_create(int device_id, const float *target, int64_t nt, int64_t stride_bytes, ppcr_scorer **out)
{
    if (!out) return fail(nullptr, PPCR_ERR_INVALID, "out is null");
    *out = nullptr;
    if (nt <= 0) return fail(nullptr, PPCR_ERR_INVALID, "ppcr_scorer_create: needs at least one target point");
    ppcr_ctx *c = nullptr;
    PPCR_TRY(ppcr_create(device_id, &c));
    auto body = [&]() -> int {
        // the grid of ppcr_nearest_sq_distances: cubic cells that hold ~3 points, one x slice per cell, one pass
        c->opt_eager_grid = 0;
        PPCR_TRY(set_target_common(c, target, false, nt, stride_bytes));
        const float *lo = c->tgt_lo, *hi = c->tgt_hi;
        double vol = 1, emax = 0;
        for (int a = 0; a < 3; a++) {
            const double e = (double)hi[a] - (double)lo[a];
            emax = std::max(emax, e);
            vol *= std::max(e, 1e-30);
        }
        double h = std::cbrt(vol * 3.0 / (double)nt);
        if (!(h > emax * 1e-4)) h = std::max(emax * 1e-4, 1e-30);  // degenerate (flat) clouds
        if (!std::isfinite(h) || !(h > 0)) h = 1.0;
        c->radius = h;
        c->opt_grid_xf = 1;
        c->opt_two_pass = 0;
        return ensure_grid(c);
    };
    const int rc = body();
    if (rc != PPCR_OK) {
        g_create_error = c->err;
        ppcr_destroy(c);
        return rc;
    }
    ppcr_scorer *s = new (std::nothrow) ppcr_scorer();
    if (!s) {
        ppcr_destroy(c);
        return fail(nullptr, PPCR_ERR_NOMEM, "out of host memory");
    }
    s->c = c;
    for (int a = 0; a < 3; a++) s->box.lo[a] = c->tgt_lo[a], s->box.hi[a] = c->tgt_hi[a];
    *out = s;
    return PPCR_OK;
}

int ppcr_scorer_set_source(ppcr_scorer *s, const float *xyz, int64_t nq, int64_t stride_bytes)
{
    if (!s) return PPCR_ERR_INVALID;
    CTX_ENTER(s->c);
    s->r_src_valid = false;  // (the refinement's sorted copy is made again at its next call)
    return set_source_common(s->c, xyz, false, nq, stride_bytes);
}

int ppcr_scorer_score(ppcr_scorer *s, const double *T, int64_t n_poses, double factor, ppcr_pose_score *scores, float *d2_out)
{
    if (!s) return PPCR_ERR_INVALID;
    ppcr_ctx *c = s->c;
    CTX_ENTER(c);
    if (!(factor >= 1) || !std::isfinite(factor)) return fail(c, PPCR_ERR_INVALID, "factor must be finite and >= 1");
    if (n_poses < 0) return fail(c, PPCR_ERR_INVALID, "n_poses must be >= 0");
    if (n_poses > 0 && (!T || !scores)) return fail(c, PPCR_ERR_INVALID, "null argument");
    if (!c->have_src) return fail(c, PPCR_ERR_STATE, "set a source before ppcr_scorer_score");
    s->last_search_ms = 0;
    s->search_events_used = 0;
    if (n_poses == 0) return PPCR_OK;
    const int64_t nq = c->ns;
    if (nq == 0) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (int64_t p = 0; p < n_poses; p++) scores[p] = ppcr_pose_score{0.0, nan, 0.0, 0, nan};
        return PPCR_OK;
    }
    PPCR_TRY(ensure_grid(c));
    // poses per chunk: d2 scratch stays bounded, and every chunk of a call uses the same cut of the scratch
    const int cap = (int)std::min<int64_t>(n_poses, std::max<int64_t>(1, std::min<int64_t>(4096, PPCR_SCORE_D2_BYTES / (4 * nq))));
    const size_t search_blocks = (size_t)nblocks(nq), stream_blocks = (size_t)nblocks(nq, kScoreSpan);
    HIP_TRY(c, s->d_poses.reserve((size_t)cap * 12));
    HIP_TRY(c, s->d_d2.reserve((size_t)cap * (size_t)nq));
    HIP_TRY(c, s->d_u32.reserve((size_t)cap * (kScoreBins * 7 + 2 * stream_blocks)));
    HIP_TRY(c, s->d_f64.reserve((size_t)cap * (search_blocks + stream_blocks + 2)));
    HIP_TRY(c, s->d_sel.reserve((size_t)cap));
    HIP_TRY(c, s->d_rcount.reserve((size_t)cap));
    HIP_TRY(c, s->d_scores.reserve((size_t)cap));
    size_t chunk = 0;
    for (int64_t p0 = 0; p0 < n_poses; p0 += cap, chunk++) {
        const int np = (int)std::min<int64_t>(cap, n_poses - p0);
        PPCR_TRY(score_chunk(s, T + 12 * p0, np, cap, factor, chunk));
        // (behind the chunk's kernels on the stream: the next chunk may overwrite the scratch)
        HIP_TRY(c, hipMemcpyAsync(scores + p0, s->d_scores.p, sizeof(ppcr_pose_score) * (size_t)np, hipMemcpyDeviceToHost, c->stream));
        if (d2_out)
            HIP_TRY(c, hipMemcpyAsync(d2_out + (size_t)p0 * (size_t)nq, s->d_d2.p, sizeof(float) * (size_t)np * (size_t)nq,
                                      hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < s->search_events_used; k++) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, s->search_events[k].first, s->search_events[k].second));
        s->last_search_ms += ms;
    }
    return PPCR_OK;
}

int ppcr_scorer_last_search_ms(ppcr_scorer *s, double *ms)
{
    if (!s || !ms) return PPCR_ERR_INVALID;
    *ms = s->last_search_ms;
    return PPCR_OK;
}

const char *ppcr_scorer_last_error(const ppcr_scorer *s) { return s ? s->c->err.c_str() : g_create_error.c_str(); }

int ppcr_scorer_destroy(ppcr_scorer *s)
{
    if (!s) return PPCR_OK;
    (void)hipSetDevice(s->c->device);
    if (s->c->stream) (void)hipStreamSynchronize(s->c->stream);
    for (auto &ev : s->search_events) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    s->d_poses.release_idle();
    s->d_f64.release_idle();
    s->d_d2.release_idle();
    s->d_u32.release_idle();
    s->d_sel.release_idle();
    s->d_rcount.release_idle();
    s->d_scores.release_idle();
    for (hipEvent_t ev : s->r_ev)
        if (ev) (void)hipEventDestroy(ev);
    s->r_tgt.release_idle();
    s->r_src.release_idle();
    s->r_cell_start.release_idle();
    s->r_partials.release_idle();
    s->r_poses.release_idle();
    s->r_frozen.release_idle();
    s->r_steps.release_idle();
    ppcr_destroy(s->c);
    delete s;
    return PPCR_OK;
}

}  // extern "C"
