// Part of the translation unit ppcr_hip.hip: one iteration's launches — K1 (associate_impl), K23, fold and solve, the
// device-paced inner steps, the host-paced solve — and the export / import of associations.

namespace {

constexpr int kAccumRows = 1;     // rows per lane of accumulate_ell_kernel
constexpr int kAccumBlock = 256;  // threads per block of accumulate_ell_kernel (fewer partial vectors to fold)

// which form of K23 serves a model: the two models the reference's CLI reaches by default are compiled in (Gaussian -u;
// t with dof 5, dim 3: v + dim = 8), any other dof takes the run-time form of the same arithmetic.  The one-pass form
// (likelihoods relative to s = 0 instead of the row's smallest s) only while that ratio stays far from underflow for
// every s the association can hold (s < radius^2 up to the float rounding of d2 and the f64 re-evaluation at another
// pose; the factor 4 on the radius covers residuals at a pose other than the one the association was made at).
struct K23Form {
    int tm;        // 0 Gaussian, 8 t with v + dim = 8, -3 t with another integer v + dim (one-pass only), -1 run-time t model
    bool onepass;
};
K23Form k23_form(const ppcr_ctx *c, const Model &md)
{
    const double s_max = 16.0 * c->radius * c->radius;
    if (md.is_normal) return K23Form{0, 0.5 * s_max < 600.0};
    // (v / (v + s))^((v + d) / 2) > 1e-250
    const bool safe = 0.5 * md.vpd * std::log10((md.v + s_max) / md.v) < 250.0;
    if (md.vpd_int == 8) return K23Form{8, safe};
    if (md.vpd_int != 0 && safe) return K23Form{-3, true};  // -d 3, -d 10, ...: integer power by squaring
    return K23Form{-1, safe};
}

template <int W>
void launch_accumulate_ell(ppcr_ctx *c, int nb, const Pose &P, const Model &md, const LoopState *loop_st)
{
#define PPCR_K23(TMc, ONEc)                                                                                        \
    accumulate_ell_kernel<W, kAccumRows, kAccumBlock, TMc, ONEc><<<nb, kAccumBlock, 0, c->stream>>>(        \
        c->nbr.p, c->cnt.p, c->src.p, c->tgt_cur(), (int)c->ns, P, md, c->partials.p, c->ell_width, loop_st)
    const K23Form f = k23_form(c, md);
    if (f.tm == 0) {
        if (f.onepass) PPCR_K23(0, true);
        else PPCR_K23(0, false);
    } else if (f.tm == 8) {
        if (f.onepass) PPCR_K23(8, true);
        else PPCR_K23(8, false);
    } else if (f.tm == -3) {
        PPCR_K23(-3, true);
    } else {
        if (f.onepass) PPCR_K23(-1, true);
        else PPCR_K23(-1, false);
    }
#undef PPCR_K23
}

int flush_pending_move(ppcr_ctx *c);

// the K1 translation unit compiled for the plan's list width (k1_width: the narrowest that holds max_neighbours)
void dispatch_tile(TileLaunch &tl)
{
    const int M = tl.plan.M;
    (M == 4 ? launch_tile_m4 : M == 5 ? launch_tile_m5 : M == 8 ? launch_tile_m8 : M == 10 ? launch_tile_m10 : M == 16 ? launch_tile_m16
     : M == 20 ? launch_tile_m20 : launch_tile_m32)(tl);
}

// workgroups of a steady-state K1 launch = slots of the partial sums it leaves when K23 is folded in
int k1_steady_slots(const ppcr_ctx *c) { return k1_steady_grid(nblocks(std::max<int64_t>(c->ns, 1), 256)); }

// The largest displacement a rigid move T (row-major [R|t]) gives any point of the target's bounding box — the source lies
// on the target, and |(R - I) p + t| is convex in p: its maximum over a box sits at a corner.  The Verlet lists are worth
// building only once this is small (ppcr_ctx::move_estimate).
double move_extent(const ppcr_ctx *c, const double T[12])
{
    double worst = 0;
    for (int k = 0; k < 8; k++) {
        const double p[3] = {(k & 1) ? c->tgt_hi[0] : c->tgt_lo[0], (k & 2) ? c->tgt_hi[1] : c->tgt_lo[1], (k & 4) ? c->tgt_hi[2] : c->tgt_lo[2]};
        double d2 = 0;
        for (int a = 0; a < 3; a++) {
            const double v = T[4 * a] * p[0] + T[4 * a + 1] * p[1] + T[4 * a + 2] * p[2] + T[4 * a + 3] - p[a];
            d2 += v * v;
        }
        worst = std::max(worst, std::sqrt(d2));
    }
    return worst;
}

// Are Verlet lists worth building (or keeping) at the association about to be enqueued?
// A list built now lives while need + path < reach, and both terms drift: the row's own m-th distance can grow by the path it
// travels, so the lists of a cloud survive while TWICE the path travelled stays inside the skin (2 x skin = grid_skin2:
// measured on the benchmark pair, tools/exp_verlet_whofails.py: the room of the tightest rows shrinks by 2 x the path).  The
// remaining path is a forecast: registrations converge geometrically, so with e = the last known move (move_lag iterations
// old) and q = the ratio of the last two known moves, the moves from this association on add up to e q^lag / (1 - q).
// Lists are built when that forecast fits the skin, and kept until it exceeds four times that (a jolt: every row would fail,
// and the list-building search costs twice the plain one).  Grids that are resident all at once (<= 1024 workgroups) are
// latency-bound — a workgroup that rebuilds a row, let alone searches, IS the launch's length — and wait until the forecast
// fits HALF the skin: the no-failure condition above taken literally (twice the path inside the skin).  No constant here is fitted to a trajectory: the skin is the lists' own
// geometry, the ratio is measured (0.9 until two moves are known, clamped to [0.3, 0.95]).
bool verlet_lists_pay_off(const ppcr_ctx *c)
{
    if (c->opt_verlet_engage >= 0) {  // a fixed threshold on the last known move (tests, experiments)
        const double engage = 1e-4 * (double)c->opt_verlet_engage * c->radius;
        return c->move_estimate <= (c->verlet_ok ? 4.0 * engage : engage);
    }
    if (!(c->move_estimate >= 0) || !std::isfinite(c->move_estimate)) return false;
    const double q = std::isfinite(c->move_ratio) ? std::min(0.95, std::max(0.3, c->move_ratio)) : 0.9;
    const double remaining = c->move_estimate * std::pow(q, (double)std::max(c->move_lag, 1)) / (1.0 - q);
    // (measured, tools/exp_verlet_sweep.py with option verlet_room: 50k / 100k / 200k rows 43.0 / 38.8 / 31.4 k it/s at half the
    //  skin against 39.2 / 35.8 / 30.9 k at all of it and 41.9 / 38.3 / 28.5 k at a quarter; 1M: all of it; the mid widths,
    //  whose K23 is its own kernel and whose failing rows cost the association less of the iteration: no difference, all of it)
    const double room = (c->opt_verlet_room >= 0 ? 0.01 * (double)c->opt_verlet_room : ((k1_steady_slots(c) > 1024 || c->max_nb > 10) ? 1.0 : 0.5)) * c->grid_skin2;
    return remaining <= (c->verlet_ok ? 4.0 * room : room);
}

// K1 (or the generic count/scan/fill path for unbounded searches and max_neighbours > 32).
// fuse_R / fuse_t (nullable): the pose the first IRLS half-step will be evaluated at; when given, the steady-state K1
// also produces that step's partial moments (c->assoc_fused, c->fused_slots) and the caller skips the K23 launch.
struct StepTicket {
    unsigned seq = 0;  // mailbox sequence number
    int nb = 0;        // partial vectors to fold
};
int prepare_fold(ppcr_ctx *c, int nslots, StepTicket &tk, FoldSolve &fs, const LoopCtl *loop);
// merge_tk (with a fuse pose): the fold-and-solve step may ride in the cleanup launch; c->assoc_folded tells whether it did
// loop (device-paced align loop only): the launches step aside while LoopState::abort is up, the fast kernel opens a new
// outer iteration in the loop state, a merged fold decides about the inner loop
int associate_impl(ppcr_ctx *c, const Mat3 *fuse_R = nullptr, const double *fuse_t = nullptr, StepTicket *merge_tk = nullptr,
                   const LoopCtl *loop = nullptr)
{
    trace_mark(c, "assoc");
    PPCR_TRY(ensure_grid(c));
    trace_mark(c, "grid");
    if (!c->src_sorted) PPCR_TRY(flush_pending_move(c));  // the one-time spatial sort reads the source
    PPCR_TRY(ensure_source_sorted(c));
    trace_mark(c, "sorted");
    invalidate_association(c);
    const int ns = (int)c->ns;
    const float r2_full = (float)(c->radius * c->radius);  // PCL: static_cast<float>(radius * radius)
    // first pass of a two-pass search: a smaller radius on a grid built for it (see ensure_grid); one pass: the radius
    const float r2 = c->reach > 1 ? std::min((float)(c->search_radius * c->search_radius), r2_full) : r2_full;
    const bool unbounded = (c->max_nb <= 0 || (int64_t)c->max_nb >= c->nt);
    const bool tiled = !unbounded && c->max_nb <= kEllMaxWidth && ns > 0;
    PendingMove pm;
    std::memset(&pm, 0, sizeof(pm));
    if (c->move_on_device && tiled) {
        // the previous iteration's transform is still on its way to the host: K1 reads it from device memory
        pm.enabled = 2;
        pm.dev = c->d_pose.p;
        c->move_on_device = false;
    } else if (c->move_pending && tiled) {
        // the deferred source move rides in this kernel's prologue
        if (!c->move_forecast_pinned) {  // (inside an align loop the forecast is the loop's: AlignJob::latch_move_forecast)
            const double now = move_extent(c, c->pending_T);
            // (two consecutive moves known: their ratio; an align loop's last transform comes with the loop's own ratio)
            if (!c->pending_from_align) c->move_ratio = (std::isfinite(c->move_estimate) && c->move_estimate > 0) ? now / c->move_estimate : std::numeric_limits<double>::quiet_NaN();
            c->move_estimate = now;
            c->move_lag = 1;
        }
        c->pending_from_align = false;
        pm.enabled = 1;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) pm.P.R[3 * a + b] = c->pending_T[4 * a + b];
            pm.P.t[a] = c->pending_T[4 * a + 3];
            pm.P.c[a] = 0;
        }
        c->move_pending = false;
    } else {
        PPCR_TRY(flush_pending_move(c));
    }
    if (!unbounded && c->max_nb <= kEllMaxWidth) {
        const int m = c->max_nb;
        HIP_TRY(c, c->nbr.reserve((size_t)m * (size_t)std::max(ns, 1)));
        HIP_TRY(c, c->cnt.reserve((size_t)std::max(ns, 1)));
        HIP_TRY(c, c->dm2.reserve((size_t)std::max(ns, 1)));
        HIP_TRY(c, c->ovf_list.reserve((size_t)k1_max_grid(nblocks(std::max(ns, 1), 256))));
        if (!c->split_clean) {
            const size_t nbk = (size_t)nblocks(std::max(ns, 1), 256);
            HIP_TRY(c, c->split_flag.reserve(nbk));
            HIP_TRY(c, c->split_list.reserve(kMaxSplit));
            HIP_TRY(c, c->split_state.reserve(3));
            HIP_TRY(c, hipMemsetAsync(c->split_flag.p, 0, nbk, c->stream));
            HIP_TRY(c, hipMemsetAsync(c->split_state.p, 0, 3 * sizeof(unsigned), c->stream));
            c->split_clean = true;
        }
        if (!c->ovf_state.p) {
            HIP_TRY(c, c->ovf_state.reserve(2));
            HIP_TRY(c, hipMemsetAsync(c->ovf_state.p, 0, 2 * sizeof(unsigned), c->stream));
        }
        // dm2 is only trusted when the source moved by nothing but the deferred rigid move applied in this
        // very kernel since the association that wrote it
        if (!tiled) c->dm2_valid = false;
        c->assoc_fused = false;
        if (ns > 0) {
            // K23 folded in: only the two compiled-in models in their one-pass form (see launch_accumulate_ell)
            FusedMoments fm;
            const FusedMoments *fuse = nullptr;
            int fuse_tm = -2;
            // (two passes: the rows are final only after the second; a cloud whose associations keep handing workgroups over
            //  — dense parts whose halos outgrow the LDS tile — leaves those rows to nn_wide_kernel, which does not fold)
            const unsigned ovf_known = c->ovf_decide_pinned ? c->ovf_decide : c->ovf_last;
            const bool many_handed_over = ovf_known != ~0u && ovf_known > (unsigned)c->opt_fuse_max_handed_over;
            if (fuse_R && c->opt_fuse_k23 && c->nt > 0 && c->reach == 1 && c->n_levels <= 1 && !many_handed_over) {
                const Model md = make_model(c);
                const K23Form form = k23_form(c, md);
                if (form.onepass && form.tm != -1) {  // the three forms compiled into K1: Gaussian, v + dim = 8, integer v + dim
                    const int slots = k1_steady_slots(c);
                    HIP_TRY(c, c->partials.reserve((size_t)slots * kNSums));
                    fm.P = make_pose(c, *fuse_R, fuse_t);
                    fm.md = md;
                    fuse_tm = form.tm;
                    fm.partials = c->partials.p;
                    fm.nslots = slots;
                    fuse = &fm;
                }
            }
            // what the plan depends on (ppcr_k1_plan.hpp); the plan itself once the Verlet mode is known
            K1Query kq{};
            kq.m = m, kq.blocks = nblocks(std::max(ns, 1), 256);
            kq.dm2_in = c->opt_temporal && c->dm2_valid, kq.short_lists = c->opt_short_lists != 0, kq.stamps = c->opt_stamps != 0;
            // (the fold-and-solve step in the same launch as the cleanup — also when several handles share the GPU: before the
            //  source-order fix of round 3 the merged launch lost there, 24.0 k it/s against 28.2 k with the small fold kernel for
            //  64 x 250k, 8 in flight; now 41.5 k against 41.0 k, and 1.33 k against 0.88 k pairs/s end to end with four pairs
            //  in flight)
            kq.k23_form = fuse_tm, kq.merge_wanted = c->opt_merge_fold && merge_tk != nullptr;
            kq.reach = c->reach, kq.n_levels = c->n_levels;
            kq.short_list = k1_wants_short_list(kq);
            kq.quiet = c->ovf_last == 0, kq.handed_last = c->ovf_last;
            // Verlet lists: the steady-state variant of a one-pass, single-level search builds them (mode 1) and from then on
            // answers from them wherever they still hold (mode 2; the other workgroups search and rebuild)
            // (widths up to 10: K23 can be folded in, 16 list slots; 11 .. 20 — the command line's default is 20 —: the
            //  mid-width variant, 32 slots, rows left to nn_wide_kernel get their lists there; a two-pass search keeps lists
            //  as well: a row's list reaches as far as ITS bound, whichever pass found it)
            // ... once they are predicted to pay off (verlet_lists_pay_off below)
            const bool calm = verlet_lists_pay_off(c);
            // A source far sparser than the target: 256 of its rows span a halo no tile holds, the tiled kernel hands every
            // block over and nn_wide_kernel answers every row (tools/exp_scan_to_map.py).  Once an association has handed
            // (nearly) all blocks over, the next ones do not try: the rows are moved and listed, nothing else (K1 60-90 us ->
            // a few); every 32nd association tries the tiles again.
            const bool list_all = ovf_known != ~0u && kq.blocks >= 16 && (double)ovf_known >= 0.9 * (double)kq.blocks && (c->assoc_counter++ % 32u) != 31u;
            const int verlet_mode = (!list_all && k1_has_steady_variant(kq) && c->opt_verlet && c->grid_skin2 > 0 && (c->reach == 1 || m > 10) &&
                                     (c->n_levels <= 1 || c->opt_verlet_levels) &&
                                     c->nt > 0 && c->ns < (1ll << 26) && (calm || c->opt_verlet == 2))
                                        ? ((c->verlet_ok && c->opt_verlet == 1) ? 2 : 1)
                                        : 0;
            if (verlet_mode) {
                const size_t rows = (size_t)std::max(ns, 1);
                HIP_TRY(c, c->vl.reserve(rows * (size_t)verlet_slots(m <= 10 ? 10 : 16)));
                HIP_TRY(c, c->vn.reserve(rows));
                HIP_TRY(c, c->vmask.reserve(rows));
                HIP_TRY(c, c->vg2.reserve(rows));
                HIP_TRY(c, c->vacc.reserve(rows));
                {   // (one byte per workgroup slot of the largest grid a K1 variant launches: two per block, or blocks + split slots)
                    const size_t slots = (size_t)k1_max_grid(kq.blocks);
                    if (c->vstreak.cap < slots) {
                        HIP_TRY(c, c->vstreak.reserve(slots));
                        HIP_TRY(c, hipMemsetAsync(c->vstreak.p, 0, slots, c->stream));
                    }
                }
                const size_t per = ((size_t)k1_steady_slots(c) + 7) / 8;
                if (!c->vcount.p || c->vorder.cap < 2 * 16 * per) {
                    HIP_TRY(c, c->vcount.reserve(64));
                    HIP_TRY(c, c->vorder.reserve(2 * 16 * per));
                    HIP_TRY(c, hipMemsetAsync(c->vcount.p, 0, 64 * sizeof(unsigned), c->stream));
                    c->verlet_order_ok = false;
                }
            }
            kq.list_all = list_all, kq.verlet_mode = verlet_mode;
            kq.verlet_rows = k1_steady_slots(c) <= 1024;  // (one residency round: a searching workgroup is the launch's length)
            kq.verlet_big_tile = (c->verlet_big_tile || c->opt_verlet_dense == 2) && m <= 10;
            const K1Plan plan = plan_k1(kq);
            // the fold-and-solve step rides in the cleanup launch: its buffers, its mailbox sequence number
            FoldSolve fs;
            if (plan.merged) PPCR_TRY(prepare_fold(c, fm.nslots, *merge_tk, fs, loop));
            ProfScope ps(c, K_NN_TOPM);
            c->ovf_parity ^= 1;
            TileLaunch tl{};
            tl.plan = plan;
            tl.stream = c->stream;
            tl.src = c->src.p, tl.ns = (int)c->ns, tl.tgt = c->tgt_sorted.p, tl.cell_start = c->cell_start.p, tl.grid = c->grid;
            tl.r2 = r2, tl.m = m;
            tl.reach = c->reach, tl.r2_full = r2_full;
            tl.levels = c->n_levels > 1 ? c->d_levels.p : nullptr, tl.n_levels = c->n_levels, tl.base_level = c->base_level;
            if (c->n_levels > 1) {
                const size_t nbk = (size_t)nblocks(std::max(ns, 1), 256);
                // two buffers of two words per block, swapped per launch with the hand-over counters (ovf_parity: rolled back
                // with recalled trains, so a launch that stepped aside is re-run on the words it would have read)
                if (!c->level_cap_clean || c->level_cap.cap < 4 * nbk) {
                    HIP_TRY(c, c->level_cap.reserve(4 * nbk));
                    HIP_TRY(c, hipMemsetD16Async(reinterpret_cast<hipDeviceptr_t>(c->level_cap.p), 0x000F, 4 * nbk, c->stream));  // cap 15, floor 0, whole
                    c->level_cap_clean = true;
                }
                tl.level_in = c->level_cap.p + (size_t)(c->ovf_parity ^ 1) * 2 * nbk;
                tl.level_out = c->level_cap.p + (size_t)c->ovf_parity * 2 * nbk;
                for (int l = 0; l < kMaxLevels; l++) tl.r2_cap[l] = c->level_r2_cap[l];
                tl.level_dbg = (c->opt_level_stats && c->level_dbg.p) ? c->level_dbg.p : nullptr;
            }
            // the rows of handed-over workgroups (and the short rows of a two-pass search) are listed for nn_wide_kernel
            if (plan.wide) {
                if (c->d_short.cap < (size_t)ns + 3) {
                    HIP_TRY(c, hipStreamSynchronize(c->stream));
                    HIP_TRY(c, c->d_short.reserve((size_t)ns + 3));
                    HIP_TRY(c, hipMemsetAsync(c->d_short.p, 0, 3 * sizeof(int), c->stream));
                }
                // (the list's counters alternate with the hand-over counters: ovf_parity, rolled back with recalled trains)
                tl.short_count = reinterpret_cast<unsigned *>(c->d_short.p) + c->ovf_parity, tl.short_list = c->d_short.p + 3;
                tl.short_seen = reinterpret_cast<unsigned *>(c->d_short.p) + 2;
            }
            if (c->d_short.p) tl.short_next = reinterpret_cast<unsigned *>(c->d_short.p) + (c->ovf_parity ^ 1);
            tl.nbr = c->nbr.p, tl.cnt = c->cnt.p, tl.dm2 = c->dm2.p;
            tl.dm2_in = kq.dm2_in ? 1 : 0;
            if (c->opt_stamps) {
                // sized from the grid this launch really has (the steady-state variant adds kMaxSplit workgroups in front, a
                // multi-level search launches two per block; the reader sums the records of exactly this grid):
                // 8 words per wave, then one word per lane (its sorted run lengths)
                const size_t nwg = (size_t)plan.grid;
                const size_t nst = (nwg * (kBlock / 64) + 64) * 8 + nwg * 256;
                if (c->d_stamps.cap < nst) {
                    HIP_TRY(c, hipStreamSynchronize(c->stream));
                    HIP_TRY(c, c->d_stamps.reserve(nst));
                }
                HIP_TRY(c, hipMemsetAsync(c->d_stamps.p, 0, nst * sizeof(unsigned long long), c->stream));
                c->stamps_wgs = nwg;
            }
            tl.stamps = c->opt_stamps ? c->d_stamps.p : nullptr;
            tl.ovf_list = c->ovf_list.p;
            tl.ovf_now = c->ovf_state.p + c->ovf_parity, tl.ovf_next = c->ovf_state.p + (c->ovf_parity ^ 1);
            tl.split_flag = c->split_flag.p, tl.split_list = c->split_list.p, tl.split_state = c->split_state.p;
            tl.pm = pm, tl.fuse = fuse, tl.fold = plan.merged ? &fs : nullptr;
            tl.loop_st = loop ? loop->st : nullptr;
            tl.verlet_mode = verlet_mode;
            if (verlet_mode) {
                tl.verlet.vl = c->vl.p, tl.verlet.vn = c->vn.p, tl.verlet.vg2 = c->vg2.p, tl.verlet.vacc = c->vacc.p;
                tl.verlet.vmask = c->vmask.p;
                // (only where a searching workgroup leaves rows to nn_wide_kernel and nothing is folded in: at the widths with K23
                //  folded in repeated searches are a passing phase of a registration that still moves — measured at 1M: a block
                //  that stopped building lists there stayed without for good, converged rate 13.5 k -> 13.0 k it/s)
                tl.verlet.streak = (m > 10 || c->n_levels > 1) ? c->vstreak.p : nullptr;
                tl.verlet.launch_tag = c->verlet_launches & 15u;
                tl.verlet.rebuilt = c->vcount.p;
                // (per launch as well: a ring of eight words, launch k counts in word k % 8 and clears word (k + 1) % 8)
                tl.verlet.searched_now = c->vcount.p + 4 + (c->verlet_launches % 8u);
                tl.verlet.searched_clear = c->vcount.p + 4 + ((c->verlet_launches + 1u) % 8u);
                {
                    // dispatch order: launch k reads order k % 2 under counters k % 3, files order (k + 1) % 2 under counters
                    // (k + 1) % 3 and clears counters (k + 2) % 3 (nobody else touches those during launch k)
                    const size_t per = ((size_t)k1_steady_slots(c) + 7) / 8;
                    const unsigned k = c->verlet_launches;
                    // (a grid that is resident all at once — four workgroups per CU, 1024 — has no dispatch order to speak of:
                    //  nothing is filed, nothing is read)
                    const bool ordered = c->opt_verlet_order && k1_steady_slots(c) > 1024;
                    const bool use = c->verlet_order_ok && ordered;
                    c->verlet_order_used = use;
                    tl.verlet.order_now = use ? c->vorder.p + (k % 2) * 16 * per : nullptr;
                    tl.verlet.count_now = c->vcount.p + 16 + (k % 3) * 16;
                    tl.verlet.order_next = ordered ? c->vorder.p + ((k + 1) % 2) * 16 * per : nullptr;
                    tl.verlet.count_next = c->vcount.p + 16 + ((k + 1) % 3) * 16;
                    tl.verlet.count_clear = c->vcount.p + 16 + ((k + 2) % 3) * 16;
                }
                tl.verlet.tgt_bytes = (unsigned)((size_t)c->nt * sizeof(float4));
                tl.verlet.skin2 = (float)c->grid_skin2;
                tl.verlet.skin_rel = c->n_levels > 1 ? (float)(2e-4 * (double)verlet_skin_units(c)) : 0.f;
            }
            tl.between = [](void *scope) { static_cast<ProfScope *>(scope)->split(K_NN_CLEANUP); };
            tl.between2 = [](void *scope) { static_cast<ProfScope *>(scope)->split(K_NN_WIDE); };
            tl.between_arg = &ps;
            trace_mark(c, "reserved");
            dispatch_tile(tl);
            trace_mark(c, "k1");
            c->verlet_ok = plan.verlet_built;
            if (plan.verlet_built) c->verlet_launches++;
            c->verlet_order_ok = plan.verlet_built;
            c->assoc_fused = plan.fused;
            c->assoc_folded = plan.merged;
            c->fused_slots = plan.fused ? fm.nslots : 0;
        }
        c->assoc_space = 1;
        PPCR_TRY(check_launch(c, "nn_fast_kernel"));
        c->dm2_valid = tiled;
        c->assoc = ppcr_ctx::ASSOC_ELL;
        c->ell_width = m;
        return PPCR_OK;
    }
    // generic path: count -> scan -> fill [-> select + compact]
    c->assoc_space = 1;
    HIP_TRY(c, c->gen_counts.reserve((size_t)ns + 1));
    HIP_TRY(c, c->gen_row_ptr.reserve((size_t)ns + 1));
    HIP_TRY(c, hipMemsetAsync(c->gen_counts.p, 0, sizeof(int) * ((size_t)ns + 1), c->stream));
    if (ns > 0) {
        ProfScope ps(c, K_NN_COUNT);
        nn_count_kernel<<<nblocks(ns), kBlock, 0, c->stream>>>(c->src.p, ns, c->tgt_sorted.p, c->cell_start.p,
                                                               c->grid, r2, c->gen_counts.p);
    }
    PPCR_TRY(check_launch(c, "nn_count_kernel"));
    auto scan = [&](int *in, int *out) -> int {
        size_t tmp_bytes = 0;
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, in, out, ns + 1, c->stream));
        HIP_TRY(c, c->cub_tmp.reserve(tmp_bytes + 16));
        ProfScope ps(c, K_NN_SCAN);
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(c->cub_tmp.p, tmp_bytes, in, out, ns + 1, c->stream));
        return PPCR_OK;
    };
    // guard int32 CSR offsets: total in-radius pairs must fit
    HIP_TRY(c, c->d_total.reserve(1));
    HIP_TRY(c, hipMemsetAsync(c->d_total.p, 0, sizeof(unsigned long long), c->stream));
    if (ns > 0) {
        ProfScope ps(c, K_COUNT_SUM);
        ell_count_sum_kernel<<<std::min(1024, nblocks(ns)), kBlock, 0, c->stream>>>(c->gen_counts.p, ns, c->d_total.p);
    }
    HIP_TRY(c, hipMemcpyAsync(c->h_total, c->d_total.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned long long total_all = *c->h_total;
    if (total_all > (unsigned long long)INT32_MAX - 1024)
        return fail(c, PPCR_ERR_INVALID, "association too large for 32-bit CSR offsets (reduce radius or set max_neighbours)");
    PPCR_TRY(scan(c->gen_counts.p, c->gen_row_ptr.p));
    HIP_TRY(c, c->gen_keys.reserve((size_t)std::max<unsigned long long>(total_all, 1)));
    HIP_TRY(c, c->gen_pos.reserve((size_t)std::max<unsigned long long>(total_all, 1)));
    if (ns > 0) {
        ProfScope ps(c, K_NN_FILL);
        nn_fill_kernel<<<nblocks(ns), kBlock, 0, c->stream>>>(c->src.p, ns, c->tgt_sorted.p, c->cell_start.p, c->grid,
                                                              r2, c->gen_row_ptr.p, c->gen_keys.p, c->gen_pos.p);
    }
    PPCR_TRY(check_launch(c, "nn_fill_kernel"));
    if (unbounded) {
        std::swap(c->row_ptr, c->gen_row_ptr);
        std::swap(c->nbr, c->gen_pos);
        c->nnz = (int64_t)total_all;
    } else {
        HIP_TRY(c, hipMemsetAsync(c->gen_counts.p, 0, sizeof(int) * ((size_t)ns + 1), c->stream));
        if (ns > 0) {
            ProfScope ps(c, K_NN_SELECT);
            nn_select_kernel<<<nblocks(ns), kBlock, 0, c->stream>>>(ns, c->gen_row_ptr.p, c->gen_keys.p, c->gen_pos.p,
                                                                    c->max_nb, c->gen_counts.p);
        }
        PPCR_TRY(check_launch(c, "nn_select_kernel"));
        HIP_TRY(c, c->row_ptr.reserve((size_t)ns + 1));
        PPCR_TRY(scan(c->gen_counts.p, c->row_ptr.p));
        HIP_TRY(c, c->nbr.reserve((size_t)std::max<unsigned long long>(total_all, 1)));
        if (ns > 0) {
            ProfScope ps(c, K_NN_COMPACT);
            csr_compact_kernel<<<nblocks(ns), kBlock, 0, c->stream>>>(ns, c->gen_row_ptr.p, c->gen_pos.p, c->row_ptr.p,
                                                                      c->nbr.p);
        }
        PPCR_TRY(check_launch(c, "csr_compact_kernel"));
        c->nnz = -1;
    }
    c->assoc = ppcr_ctx::ASSOC_CSR;
    return PPCR_OK;
}

int ensure_nnz(ppcr_ctx *c)
{
    if (c->assoc == ppcr_ctx::ASSOC_NONE) return fail(c, PPCR_ERR_STATE, "no association (call ppcr_associate or ppcr_set_association)");
    if (c->nnz >= 0) return PPCR_OK;
    const int ns = (int)c->ns;
    if (c->assoc == ppcr_ctx::ASSOC_CSR) {
        int last = 0;
        HIP_TRY(c, hipMemcpyAsync(&last, c->row_ptr.p + ns, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->nnz = last;
        return PPCR_OK;
    }
    HIP_TRY(c, c->d_total.reserve(1));
    HIP_TRY(c, hipMemsetAsync(c->d_total.p, 0, sizeof(unsigned long long), c->stream));
    if (ns > 0) {
        ProfScope ps(c, K_COUNT_SUM);
        ell_count_sum_kernel<<<std::min(1024, nblocks(ns)), kBlock, 0, c->stream>>>(c->cnt.p, ns, c->d_total.p);
    }
    PPCR_TRY(check_launch(c, "ell_count_sum_kernel"));
    HIP_TRY(c, hipMemcpyAsync(c->h_total, c->d_total.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->nnz = (int64_t)*c->h_total;
    return PPCR_OK;
}

// download the w lane (original index) of a float4 cloud
int download_order(ppcr_ctx *c, const float4 *pts, int64_t n, std::vector<int> &order)
{
    std::vector<float4> tmp((size_t)n);
    if (n > 0) {
        HIP_TRY(c, hipMemcpyAsync(tmp.data(), pts, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    order.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        int v;
        std::memcpy(&v, &tmp[(size_t)i].w, sizeof(int));
        order[(size_t)i] = v;
    }
    return PPCR_OK;
}

// Build the CSR view (original row order, ascending original columns) of a device-made association
int build_csr_cache(ppcr_ctx *c)
{
    if (c->csr_cache_valid) return PPCR_OK;
    PPCR_TRY(ensure_nnz(c));
    const int64_t ns = c->ns;
    std::vector<int> src_order, tgt_order;
    PPCR_TRY(download_order(c, c->src.p, ns, src_order));
    PPCR_TRY(download_order(c, c->tgt_cur(), c->nt, tgt_order));
    std::vector<int> h_nbr, h_cnt, h_rp;
    if (c->assoc == ppcr_ctx::ASSOC_ELL) {
        h_nbr.resize((size_t)c->ell_width * (size_t)ns);
        h_cnt.resize((size_t)ns);
        if (ns > 0) {
            HIP_TRY(c, hipMemcpyAsync(h_nbr.data(), c->nbr.p, h_nbr.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(h_cnt.data(), c->cnt.p, h_cnt.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    } else {
        h_rp.resize((size_t)ns + 1);
        h_nbr.resize((size_t)c->nnz);
        HIP_TRY(c, hipMemcpyAsync(h_rp.data(), c->row_ptr.p, h_rp.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (c->nnz > 0)
            HIP_TRY(c, hipMemcpyAsync(h_nbr.data(), c->nbr.p, h_nbr.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    auto row_count = [&](int64_t r) { return c->assoc == ppcr_ctx::ASSOC_ELL ? h_cnt[(size_t)r] : h_rp[(size_t)r + 1] - h_rp[(size_t)r]; };
    auto slot_of = [&](int64_t r, int k) -> size_t {
        return c->assoc == ppcr_ctx::ASSOC_ELL ? (size_t)k * (size_t)ns + (size_t)r : (size_t)h_rp[(size_t)r] + (size_t)k;
    };
    c->h_csr_row_ptr.assign((size_t)ns + 1, 0);
    for (int64_t r = 0; r < ns; r++) c->h_csr_row_ptr[(size_t)src_order[(size_t)r] + 1] = row_count(r);
    for (int64_t i = 0; i < ns; i++) c->h_csr_row_ptr[(size_t)i + 1] += c->h_csr_row_ptr[(size_t)i];
    const size_t nnz = (size_t)c->h_csr_row_ptr[(size_t)ns];
    c->h_csr_col.resize(nnz);
    c->h_csr_slot.resize(nnz);
    std::vector<std::pair<int, size_t>> row;
    for (int64_t r = 0; r < ns; r++) {
        const int n = row_count(r);
        row.clear();
        for (int k = 0; k < n; k++) {
            const size_t sl = slot_of(r, k);
            row.emplace_back(tgt_order[(size_t)h_nbr[sl]], sl);
        }
        std::sort(row.begin(), row.end());
        const size_t base = (size_t)c->h_csr_row_ptr[(size_t)src_order[(size_t)r]];
        for (int k = 0; k < n; k++) {
            c->h_csr_col[base + k] = row[(size_t)k].first;
            c->h_csr_slot[base + k] = row[(size_t)k].second;
        }
    }
    c->csr_cache_valid = true;
    return PPCR_OK;
}

// One IRLS half-step on the device: K23 (weights + moments at the pose R, t) -> fold -> closed-form solve.
struct StepResult {
    double sums[PPCR_NSUMS];
    double T[12];      // minimiser for these moments
    double cost;       // 0.5 * sum w |y - R x - t|^2 at T (Ceres' convention)
    bool degenerate;   // no weight mass: T = identity
    // device-paced inner loop (MailboxStatus other than kStepResult)
    unsigned status = kStepResult;
    int steps = 0;          // IRLS steps the device took in this outer iteration
    double cost_init = 0;   // 0.5 * sum w s at the pose the outer iteration started from
};
// buffers and arguments of one fold-and-solve step; draws the step's mailbox sequence number
int prepare_fold(ppcr_ctx *c, int nslots, StepTicket &tk, FoldSolve &fs, const LoopCtl *loop)
{
    HIP_TRY(c, c->d_sums.reserve(kNSums));
    HIP_TRY(c, c->d_pose.reserve(1));
    if (!c->d_ticket.p) {
        HIP_TRY(c, c->d_ticket.reserve(2));
        HIP_TRY(c, hipMemsetAsync(c->d_ticket.p, 0, 2 * sizeof(unsigned), c->stream));
    }
    tk.seq = ++c->mbox_seq;
    tk.nb = nslots;
    fs.partials = c->partials.p;
    fs.nslots = nslots;
    fs.sums = c->d_sums.p;
    fs.origin = make_double3(c->origin[0], c->origin[1], c->origin[2]);
    fs.pose_out = c->d_pose.p;
    fs.mbox = c->d_mbox + (tk.seq % kMailboxRing);
    fs.ticket = c->d_ticket.p;
    fs.seq = tk.seq;
    fs.handed_over = c->ovf_state.p ? c->ovf_state.p + c->ovf_parity : nullptr;
    fs.split_list = c->split_clean ? c->split_list.p : nullptr;
    fs.split_flag = c->split_clean ? c->split_flag.p : nullptr;
    fs.split_total = c->split_clean ? c->split_state.p : nullptr;
    fs.split_visible = c->split_clean ? c->split_state.p + 1 : nullptr;
    fs.split_rebuilt = c->split_clean ? c->split_state.p + 2 : nullptr;
    fs.split_nblocks = nblocks(std::max((int)c->ns, 1), 256);
    fs.dbg = c->opt_fold_stamps ? c->d_fold_dbg.p : nullptr;
    if (loop) {
        fs.loop = *loop;
    } else {
        fs.loop.st = nullptr;  // host-paced: every step is published, the host decides
        fs.loop.f_tol = 0.0;
        fs.loop.max_steps = 0;
        fs.loop.first = fs.loop.last_dev = 0;
    }
    return PPCR_OK;
}

// enqueue K23 + fold (+ solve); nothing here waits for the device.  use_fused: the association just made already
// produced the partial moments for this pose (associate_impl with a fuse pose): only the fold and the solve remain.
int launch_step(ppcr_ctx *c, const Mat3 &R, const double t[3], StepTicket &tk, bool use_fused = false,
                const LoopCtl *loop = nullptr)
{
    if (c->assoc == ppcr_ctx::ASSOC_NONE) return fail(c, PPCR_ERR_STATE, "no association (call ppcr_associate or ppcr_set_association)");
    if (!c->origin_valid) {
        // set_association path without a grid: origin = 0 is fine for the exact-association API,
        // but prefer the target bounding-box centre when a grid has been built
        c->origin[0] = c->origin[1] = c->origin[2] = 0;
    }
    const int ns = (int)c->ns;
    const Pose P = make_pose(c, R, t);
    const Model md = make_model(c);
    const bool ell_rows = c->assoc == ppcr_ctx::ASSOC_ELL && c->nt > 0;
    // the ELL kernel covers every row exactly once (kAccumRows rows per lane); the generic one grid-strides
    const int nb = use_fused ? c->fused_slots
                             : (ell_rows ? std::max(1, nblocks(ns, kAccumBlock * kAccumRows)) : std::max(1, std::min(kAccumMaxBlocks, nblocks(ns))));
    HIP_TRY(c, c->partials.reserve((size_t)nb * kNSums));
    HIP_TRY(c, c->d_sums.reserve(kNSums));
    const LoopState *loop_st = loop ? loop->st : nullptr;
    if (!use_fused) {
        ProfScope ps(c, K_ACCUMULATE);
        if (c->assoc == ppcr_ctx::ASSOC_ELL && c->nt > 0) {
            const int w = c->ell_width;
            if (w <= 4) launch_accumulate_ell<4>(c, nb, P, md, loop_st);
            else if (w <= 8) launch_accumulate_ell<8>(c, nb, P, md, loop_st);
            else if (w <= 10) launch_accumulate_ell<10>(c, nb, P, md, loop_st);
            else if (w <= 16) launch_accumulate_ell<16>(c, nb, P, md, loop_st);
            else if (w <= 20) launch_accumulate_ell<20>(c, nb, P, md, loop_st);
            else launch_accumulate_ell<32>(c, nb, P, md, loop_st);
        } else if (c->assoc == ppcr_ctx::ASSOC_ELL) {
            EllAssoc a{c->nbr.p, c->cnt.p, ns};
            accumulate_kernel<EllAssoc><<<nb, kBlock, 0, c->stream>>>(a, c->src.p, c->tgt_cur(), ns, P, md, c->partials.p);
        } else {
            CsrAssoc a{c->nbr.p, c->row_ptr.p};
            accumulate_kernel<CsrAssoc><<<nb, kBlock, 0, c->stream>>>(a, c->src.p, c->tgt_cur(), ns, P, md, c->partials.p);
        }
    }
    PPCR_TRY(check_launch(c, "accumulate_kernel"));
    tk.nb = nb;
    // fold + solve on the device; moments, transform and cost arrive in the host mailbox ring
    FoldSolve fs;
    PPCR_TRY(prepare_fold(c, nb, tk, fs, loop));
    const auto tl0 = std::chrono::steady_clock::now();
    {
        ProfScope ps(c, K_REDUCE);
        reduce_solve_kernel<<<kNSums, kBlock, 0, c->stream>>>(fs);
    }
    PPCR_TRY(check_launch(c, "reduce_solve_kernel"));
    c->dbg_host[6] = std::max(c->dbg_host[6], std::chrono::duration<double>(std::chrono::steady_clock::now() - tl0).count());
    return PPCR_OK;
}

// has that step's result reached the host mailbox yet?  (never blocks)
bool step_arrived(const ppcr_ctx *c, const StepTicket &tk)
{
    const HostMailbox *mb = c->h_mbox + (tk.seq % kMailboxRing);
    return __atomic_load_n(&mb->seq, __ATOMIC_ACQUIRE) == tk.seq;
}

// wait for that step and fetch its result
int collect_step(ppcr_ctx *c, const StepTicket &tk, StepResult &out)
{
    const HostMailbox *mb = c->h_mbox + (tk.seq % kMailboxRing);
    volatile const unsigned *flag = &mb->seq;
    bool arrived = false;
    const auto tw0 = std::chrono::steady_clock::now();
    for (long spin = 0; spin < 200000000L; spin++) {  // ~ seconds; a fault on the device ends up below
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == tk.seq) {
            arrived = true;
            break;
        }
        // a short wait is spun through (an iteration lasts ~0.1 ms); past that the core is offered to whoever
        // else wants it, so many handles driven from more threads than cores do not starve each other
        if (spin > 4096) std::this_thread::yield();
        // (a device fault must not take seconds to surface: look at the stream every 2^16 polls, a few milliseconds)
        if ((spin & 0xFFFF) == 0xFFFF && hipStreamQuery(c->stream) != hipErrorNotReady) {
            arrived = __atomic_load_n(flag, __ATOMIC_ACQUIRE) == tk.seq;
            break;
        }
    }
    if (!arrived) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != tk.seq) return fail(c, PPCR_ERR_HIP, "moment mailbox never arrived");
    }
    for (int j = 0; j < kNSums; j++) out.sums[j] = mb->sums[j];
    for (int j = 0; j < 12; j++) out.T[j] = mb->T[j];
    out.cost = mb->cost;
    out.degenerate = mb->degenerate != 0;
    out.status = mb->status;
    out.steps = mb->steps;
    out.cost_init = mb->cost_init;
    if (out.status != kLaunchSkipped) {
        c->ovf_last = mb->handed_over;
        c->dbg_host[7] += (double)mb->handed_over;  // workgroups the associations of this ppcr_align handed to the cleanup kernel
    }
    const double w = std::chrono::duration<double>(std::chrono::steady_clock::now() - tw0).count();
    c->dbg_host[0] += 1;
    c->dbg_host[1] += w;
    c->dbg_host[2] = std::max(c->dbg_host[2], w);
    return PPCR_OK;
}

// buffers of the device-paced loop (once per handle)
int ensure_loop_state(ppcr_ctx *c)
{
    if (!c->d_loop.p) {
        HIP_TRY(c, c->d_loop.reserve(1));
        HIP_TRY(c, hipMemsetAsync(c->d_loop.p, 0, sizeof(LoopState), c->stream));
    }
    {
        // sized for the largest inner-step launch; words stamped with sequence numbers, so cleared only when (re)allocated
        const size_t want = 2 + (size_t)kMaxDevSteps * kInnerMaxG;
        if (c->d_inner_ctl.cap < want) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, c->d_inner_ctl.reserve(want));
            HIP_TRY(c, hipMemsetAsync(c->d_inner_ctl.p, 0, c->d_inner_ctl.cap * sizeof(unsigned), c->stream));
        }
    }
    if (!c->d_ticket.p) {
        HIP_TRY(c, c->d_ticket.reserve(2));
        HIP_TRY(c, hipMemsetAsync(c->d_ticket.p, 0, 2 * sizeof(unsigned), c->stream));
    }
    HIP_TRY(c, c->d_pose.reserve(1));
    return PPCR_OK;
}

// The later IRLS steps of the current outer iteration as ONE launch the device walks through on its own
// (inner_steps_kernel): step 1 was enqueued with loop control by the caller; its mailbox slot (tk.seq) is the one the
// iteration's last step publishes in.
template <int W>
void launch_inner_w(ppcr_ctx *c, const InnerArgs &a, const K23Form &f, int grid)
{
#define PPCR_INNER(TMc, ONEc) inner_steps_kernel<W, TMc, ONEc><<<grid, kBlock, 0, c->stream>>>(a)
    if (f.tm == 0) {
        if (f.onepass) PPCR_INNER(0, true);
        else PPCR_INNER(0, false);
    } else if (f.tm == 8) {
        if (f.onepass) PPCR_INNER(8, true);
        else PPCR_INNER(8, false);
    } else if (f.tm == -3) {
        PPCR_INNER(-3, true);
    } else {
        if (f.onepass) PPCR_INNER(-1, true);
        else PPCR_INNER(-1, false);
    }
#undef PPCR_INNER
}
int launch_inner(ppcr_ctx *c, const StepTicket &tk, const LoopCtl &loop, int n_dev_steps)
{
    if (n_dev_steps <= 0) return PPCR_OK;
    if (c->assoc != ppcr_ctx::ASSOC_ELL || c->nt <= 0) return fail(c, PPCR_ERR_STATE, "internal: device-paced inner steps need an ELL association");
    const int ns = (int)c->ns;
    const int ntiles = nblocks(ns, kBlock);
    // about five K23 workgroups per CU at a time, every one with the same number of tiles (+-1): the launch carries
    // n_dev_steps * (G + 19) workgroups that all have to start and look at the loop state even when step 1 ended the
    // loop (the common case), so G is not simply ntiles (3 x 3926 idle workgroups cost ~15 us per iteration at 1M)
    // (and one step's G + 19 workgroups must be resident TOGETHER — five per CU, 1280 — or the step takes two rounds:
    //  1303 + 19 of them cost 57 us per step, 977 + 19 cost 48)
    const int per_wg = std::max(1, (ntiles + kInnerStepWgs - 1) / kInnerStepWgs);
    int G = std::max(1, std::min((ntiles + per_wg - 1) / per_wg, kInnerMaxG));
    if (per_wg > 1) G = std::min((G + 7) & ~7, kInnerMaxG);  // (a multiple of eight: the kernel's XCD-aware tile map)
    HIP_TRY(c, c->partials.reserve((size_t)std::max(G, k1_steady_slots(c)) * kNSums));
    InnerArgs a;
    std::memset(&a, 0, sizeof(a));
    a.nbr = c->nbr.p, a.cnt = c->cnt.p, a.src = c->src.p, a.tgt = c->tgt_cur();
    a.ns = ns, a.width = c->ell_width;
    a.md = make_model(c);
    InnerConst ic;
    std::memset(&ic, 0, sizeof(ic));
    StepTicket same = tk;
    const unsigned seq_keep = c->mbox_seq;
    PPCR_TRY(prepare_fold(c, G, same, ic.fs, &loop));  // (draws a sequence number: handed back — the steps share tk.seq)
    c->mbox_seq = seq_keep;
    ic.fs.seq = 0, ic.fs.mbox = nullptr, ic.fs.handed_over = nullptr;  // per launch
    ic.fs.loop.first = 0, ic.fs.loop.last_dev = 0;                     // per step
    ic.flags = c->d_inner_ctl.p + 2, ic.step_done = reinterpret_cast<unsigned long long *>(c->d_inner_ctl.p);
    ic.mbox_ring = c->d_mbox, ic.mbox_slots = kMailboxRing;
    ic.ovf_state = c->ovf_state.p;
    ic.G = G;
    HIP_TRY(c, c->d_inner_const.reserve(1));
    if (!c->inner_const_valid || std::memcmp(&ic, &c->h_inner_const, sizeof(ic)) != 0) {
        // (once per change of buffers or loop control: launches already in flight read the old contents)
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->h_inner_const = ic;
        HIP_TRY(c, hipMemcpy(c->d_inner_const.p, &c->h_inner_const, sizeof(ic), hipMemcpyHostToDevice));
        c->inner_const_valid = true;
    }
    a.ic = c->d_inner_const.p;
    a.seq = tk.seq;
    a.ovf_index = c->ovf_parity;
    a.n_steps = n_dev_steps;
    const K23Form f = k23_form(c, a.md);
    const int grid = n_dev_steps * (G + kInnerFoldSlots);
    {
        ProfScope ps(c, K_INNER);
        const int w = c->ell_width;
        if (w <= 10) launch_inner_w<10>(c, a, f, grid);
        else if (w <= 16) launch_inner_w<16>(c, a, f, grid);
        else if (w <= 20) launch_inner_w<20>(c, a, f, grid);  // (the command line's default width)
        else launch_inner_w<32>(c, a, f, grid);
    }
    return check_launch(c, "inner_steps_kernel");
}

// What follows an outer iteration inside the device-paced loop: the companion cloud moves (in place) by the transform in
// *d_pose, and the per-iteration reports are formed (track_kernel).  report_flags: PPCR_REPORT_*; the means arrive in
// the report ring under sequence number `seq`.
int launch_track(ppcr_ctx *c, unsigned seq, int report_flags)
{
    const bool want_truth = (report_flags & PPCR_REPORT_TRUTH) != 0, want_moved = (report_flags & PPCR_REPORT_MOVED) != 0;
    if (!c->have_companion && !want_truth && !want_moved) return PPCR_OK;
    TrackArgs a;
    std::memset(&a, 0, sizeof(a));
    if (c->have_companion) {
        a.cloud = c->companion.p, a.n = (int)c->n_companion, a.sorted_source = 0, a.write_back = 1;
    } else {
        a.cloud = c->src.p, a.n = (int)c->ns, a.sorted_source = 1, a.write_back = 0;
    }
    if (want_truth) {
        if (!c->have_ground_truth) return fail(c, PPCR_ERR_STATE, "ground truth cloud not set");
        if ((int64_t)a.n != c->n_ground_truth) return fail(c, PPCR_ERR_INVALID, "ground truth and source clouds differ in size");
        a.truth = c->ground_truth.p;
    }
    a.want_moved = want_moved ? 1 : 0;
    a.pose = c->d_pose.p;
    const int nb = std::max(1, std::min(1024, nblocks(a.n)));  // the grid of mean_distance(): same block sums
    HIP_TRY(c, c->track_part.reserve((size_t)2 * nb));
    if (!c->track_ticket.p) {
        HIP_TRY(c, c->track_ticket.reserve(1));
        HIP_TRY(c, hipMemsetAsync(c->track_ticket.p, 0, sizeof(unsigned), c->stream));
    }
    a.part = c->track_part.p;
    a.ticket = c->track_ticket.p;
    a.out = (want_truth || want_moved) ? c->d_report + (seq % kMailboxRing) : nullptr;
    a.seq = seq;
    a.st = c->d_loop.p;
    {
        ProfScope ps(c, K_TRACK);
        track_kernel<<<nb, kBlock, 0, c->stream>>>(a);
    }
    return check_launch(c, "track_kernel");
}

// wait for the report of iteration `seq` (it trails the iteration's mailbox slot by one small kernel)
int collect_report(ppcr_ctx *c, unsigned seq, double *mse_truth, double *moved)
{
    const HostReport *r = c->h_report + (seq % kMailboxRing);
    bool arrived = false;
    for (long spin = 0; spin < 200000000L; spin++) {
        if (__atomic_load_n(&r->seq, __ATOMIC_ACQUIRE) == seq) {
            arrived = true;
            break;
        }
        if (spin > 4096) std::this_thread::yield();
        if ((spin & 0xFFFF) == 0xFFFF && hipStreamQuery(c->stream) != hipErrorNotReady) {
            arrived = __atomic_load_n(&r->seq, __ATOMIC_ACQUIRE) == seq;
            break;
        }
    }
    if (!arrived) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (__atomic_load_n(&r->seq, __ATOMIC_ACQUIRE) != seq) return fail(c, PPCR_ERR_HIP, "iteration report never arrived");
    }
    *mse_truth = r->mse_truth;
    *moved = r->moved;
    return PPCR_OK;
}

int run_accumulate(ppcr_ctx *c, const Mat3 &R, const double t[3], double sums[PPCR_NSUMS])
{
    PPCR_TRY(flush_pending_move(c));
    StepTicket tk;
    StepResult res;
    PPCR_TRY(launch_step(c, R, t, tk));
    PPCR_TRY(collect_step(c, tk, res));
    std::memcpy(sums, res.sums, sizeof(res.sums));
    return PPCR_OK;
}

int apply_transform_now(ppcr_ctx *c, const double T[12]);

// make the device copy of the source current (a move deferred to the next tiled K1 is applied now)
int flush_pending_move(ppcr_ctx *c)
{
    if (c->move_on_device) return fail(c, PPCR_ERR_STATE, "internal: a device-resident move is pending outside the align loop");
    if (!c->move_pending) return PPCR_OK;
    c->move_pending = false;
    return apply_transform_now(c, c->pending_T);
}

// move the source; when `defer` the move rides along with the next tiled association instead of its own launch
int apply_transform_impl(ppcr_ctx *c, const double T[12], bool defer = false, bool move_companion = true)
{
    if (!c->have_src) return fail(c, PPCR_ERR_STATE, "source cloud not set");
    PPCR_TRY(flush_pending_move(c));
    if (move_companion && c->have_companion && c->n_companion > 0) {
        // the full-resolution copy moves with the same f64 -> f32 arithmetic, at once (it is off the hot path)
        Pose P;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) P.R[3 * a + b] = T[4 * a + b];
            P.t[a] = T[4 * a + 3];
            P.c[a] = 0;
        }
        ProfScope ps(c, K_TRANSFORM);
        transform_kernel<<<nblocks(c->n_companion), kBlock, 0, c->stream>>>(c->companion.p, (int)c->n_companion, P);
    }
    if (defer) {
        std::memcpy(c->pending_T, T, sizeof(c->pending_T));
        c->move_pending = true;
        c->pending_from_align = false;  // (AlignJob raises it after its own call)
        return PPCR_OK;
    }
    return apply_transform_now(c, T);
}

int apply_transform_now(ppcr_ctx *c, const double T[12])
{
    c->dm2_valid = false;  // the source moved outside a tiled K1: the temporal cut-off starts over
    c->pending_from_align = false;
    Pose P;
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) P.R[3 * a + b] = T[4 * a + b];
        P.t[a] = T[4 * a + 3];
        P.c[a] = 0;
    }
    if (c->ns > 0) {
        ProfScope ps(c, K_TRANSFORM);
        transform_kernel<<<nblocks(c->ns), kBlock, 0, c->stream>>>(c->src.p, (int)c->ns, P);
    }
    return check_launch(c, "transform_kernel");
}

// The IRLS loop both routes to the moments share: launch(R, t, ticket) enqueues the kernels that leave the partial moments
// at that pose and the fold-and-solve step behind them (launch_step for a stored association, launch_radius_step for the
// implicit unbounded one); the host only compares costs
template <class Launch>
int irls_loop(ppcr_ctx *c, const double q0[4], const double t0[3], int max_steps, double f_tol, double T_out[12],
              double cost_out[2], int *steps_out, Launch &&launch)
{
    const double qn = q0[0] * q0[0] + q0[1] * q0[1] + q0[2] * q0[2] + q0[3] * q0[3];
    if (!(qn > 0) || !std::isfinite(qn)) return fail(c, PPCR_ERR_INVALID, "initial rotation quaternion has zero or non-finite norm");
    PPCR_TRY(flush_pending_move(c));
    Mat3 R = quat_to_rot(q0);
    Vec3 t{{t0[0], t0[1], t0[2]}};
    StepTicket tk;
    StepResult res;
    PPCR_TRY(launch(R, t.v, tk));
    PPCR_TRY(collect_step(c, tk, res));
    double cost_old = 0.5 * res.sums[16];
    cost_out[0] = cost_out[1] = cost_old;
    int steps = 0;
    if (max_steps < 1) max_steps = 1;
    for (;;) {
        const double fc = res.degenerate ? cost_old : res.cost;
        steps++;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) R.m[a][b] = res.T[4 * a + b];
            t[a] = res.T[4 * a + 3];
        }
        cost_out[1] = fc;
        if (res.degenerate || steps >= max_steps) break;
        // a decrease below the rounding floor of the moment-based cost (eps * (Sxx + Syy)) is no decrease
        if ((cost_old - fc) <= std::max(f_tol * cost_old, 1e-14 * 0.5 * (res.sums[17] + res.sums[18]))) break;
        PPCR_TRY(launch(R, t.v, tk));
        PPCR_TRY(collect_step(c, tk, res));
        cost_old = 0.5 * res.sums[16];
    }
    // transformation(): normalised quaternion -> rotation (..._iteration.hpp:59-67); R is already
    // orthonormal to rounding so the round trip through a quaternion is not needed here
    pack_T(R, t, T_out);
    if (steps_out) *steps_out = steps;
    return PPCR_OK;
}

// IRLS on the current association (see ppcr_solve in ppcr.h): every half-step is K23 -> fold -> solve on the device
int solve_impl(ppcr_ctx *c, const double q0[4], const double t0[3], int max_steps, double f_tol, double T_out[12],
               double cost_out[2], int *steps_out)
{
    return irls_loop(c, q0, t0, max_steps, f_tol, T_out, cost_out, steps_out,
                     [c](const Mat3 &R, const double t[3], StepTicket &tk) { return launch_step(c, R, t, tk); });
}

}  // namespace
