// Part of the translation unit ppcr_hip.hip: the registration loop (AlignJob: run-ahead, mailboxes, reports) and its
// entry points ppcr_align / ppcr_align_report, diagnostics, profiling.

// ---- reporting clouds (SURVEY 8(f) row 3): helpers shared by the align loop and the report entry points ----------------------------------------------------
namespace {

// the cloud the reference reports on: the full-resolution companion when one is set, else the source itself
struct Tracked {
    const float4 *p;
    int64_t n;
    int sorted;  // 1: the handle's sorted source (w lane = caller's index)
};
int tracked_cloud(ppcr_ctx *c, Tracked &t)
{
    if (c->have_companion) {
        t = Tracked{c->companion.p, c->n_companion, 0};
        return PPCR_OK;
    }
    if (!c->have_src) return fail(c, PPCR_ERR_STATE, "source cloud not set");
    PPCR_TRY(flush_pending_move(c));
    t = Tracked{c->src.p, c->ns, 1};
    return PPCR_OK;
}

int mean_distance(ppcr_ctx *c, const Tracked &t, const float4 *other, double *out)
{
    if (t.n == 0) {
        *out = std::numeric_limits<double>::quiet_NaN();  // 0 / 0, as the reference's loop would produce
        return PPCR_OK;
    }
    const int nb = std::min(1024, nblocks(t.n));
    HIP_TRY(c, c->mse_part.reserve((size_t)nb));
    mean_distance_kernel<<<nb, kBlock, 0, c->stream>>>(t.p, (int)t.n, other, t.sorted, c->mse_part.p);
    PPCR_TRY(check_launch(c, "mean_distance_kernel"));
    std::vector<double> h((size_t)nb);
    HIP_TRY(c, hipMemcpyAsync(h.data(), c->mse_part.p, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double sum = 0;
    for (double v : h) sum += v;
    *out = sum / (double)t.n;
    return PPCR_OK;
}

int snapshot_tracked(ppcr_ctx *c, const Tracked &t)
{
    HIP_TRY(c, c->previous.reserve((size_t)std::max<int64_t>(t.n, 1)));
    if (t.n > 0) snapshot_kernel<<<nblocks(t.n), kBlock, 0, c->stream>>>(t.p, (int)t.n, t.sorted, c->previous.p);
    PPCR_TRY(check_launch(c, "snapshot_kernel"));
    c->n_previous = t.n;
    c->have_previous = true;
    return PPCR_OK;
}

}  // namespace

namespace {

// One align() call as a resumable state machine, so that ONE host thread can keep several handles busy (each handle
// has its own stream; the device paces itself through the fold-and-solve lanes and PendingMove::dev).
//
// Pipelined mode (every bounded search on the tiled kernels): the device runs one iteration AHEAD of the host.  An
// outer iteration is a fixed train of launches — association (K23 of the first IRLS step folded in), fold-and-solve,
// the later IRLS steps of the inner loop as one device-walked launch (inner_steps_kernel; only when inner_steps > 1),
// the companion move / per-iteration reports (track_kernel; only when there is something to move or report) — and
// the lane that solves a step decides on the device whether the inner loop is over (LoopCtl: the test of solve_impl).
// Iteration k + 1 is enqueued before the host has seen iteration k — but only when hasConverged() cannot stop in
// between whatever the cost of iteration k turns out to be: the cap is not reached and the idle count is within the
// patience.  The rule therefore stays exact: nothing speculative is ever enqueued.
// Should an inner loop need more steps than were enqueued for the device (option inner_dev_steps), the device raises
// LoopState::abort, everything enqueued behind steps aside untouched, and the host finishes that iteration one step
// at a time (take_over) before the train continues.
struct AlignJob {
    ppcr_ctx *c = nullptr;
    int n_iter = 0, inner_steps = 1;
    double thresh = 0, patience = 0, f_tol = 1e-5;
    double q0[4] = {1, 0, 0, 0}, t0[3] = {0, 0, 0};
    double *history = nullptr, *costs = nullptr;
    int32_t *steps = nullptr;
    int report_flags = 0;                   // PPCR_REPORT_*
    ppcr_iteration_fn on_iteration = nullptr;
    void *user = nullptr;
    ppcr_stop_rule rule = {0, 0, 0.0};  // hasConverged(), shared with the C++ class (ppcr.h)
    double Tcum[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double T_last[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    Mat3 R0 = Mat3::identity();
    StepTicket in_flight[kMailboxRing];
    int enq = 0, done = 0;
    bool pipelined = false, finished = false;
    unsigned handed_over_of[kMailboxRing] = {~0u, ~0u, ~0u, ~0u};  // per iteration in flight / just consumed (index % ring)
    bool verlet_after[kMailboxRing] = {false, false, false, false};  // c->verlet_ok as each train's association left it
    // the move estimate each consumed iteration left (index % ring) and the one this call's first association went by: which
    // association builds / keeps Verlet lists goes by the estimate of the iteration kMaxAhead back — consumed for sure —
    // so the sequence of kernels depends on the iteration index alone, not on when results happen to reach this thread
    double estimate_of[kMailboxRing] = {0, 0, 0, 0}, estimate_entry = 0;
    double ratio_of[kMailboxRing] = {0, 0, 0, 0}, ratio_entry = 0, estimate_last = std::numeric_limits<double>::quiet_NaN();
    int base_iteration = 0;  // iterations of the align calls this one continues (ppcr_ctx::al_iterations; 0: a fresh start)
    static_assert(kMailboxRing == 4, "initialiser above");
    int max_steps = 1, n_dev_steps = 0;
    int steps_of[kMailboxRing] = {0, 0, 0, 0};  // IRLS steps each consumed iteration took (index % ring)
    LoopCtl loop{};
    Pose handback{};  // take_over: the pose the host solved, on its way back to the device

    int validate()
    {
        if (!c) return PPCR_ERR_INVALID;
        HIP_TRY(c, hipSetDevice(c->device));
        // n_iter < 0 means "no iteration cap" in the reference (cc:140 never fires): legal, but then the per-iteration
        // arrays cannot be sized by the caller
        if (n_iter < 0 && (history || costs || steps))
            return fail(c, PPCR_ERR_INVALID, "ppcr_align: n_iter < 0 (no iteration cap) needs history, costs and steps to be NULL");
        if (n_iter < 0 && !(thresh > 0))
            return fail(c, PPCR_ERR_INVALID, "ppcr_align: n_iter < 0 (no iteration cap) needs cost_drop_thresh > 0, or the loop never ends");
        if (!c->have_src || !c->have_tgt) return fail(c, PPCR_ERR_STATE, "set source and target before ppcr_align");
        const double qn = q0[0] * q0[0] + q0[1] * q0[1] + q0[2] * q0[2] + q0[3] * q0[3];
        if (!(qn > 0) || !std::isfinite(qn)) return fail(c, PPCR_ERR_INVALID, "initial rotation quaternion has zero or non-finite norm");
        if ((report_flags & PPCR_REPORT_TRUTH) && !c->have_ground_truth) return fail(c, PPCR_ERR_STATE, "ground truth cloud not set");
        if (report_flags & PPCR_REPORT_TRUTH) {
            const int64_t n_tracked = c->have_companion ? c->n_companion : c->ns;
            if (n_tracked != c->n_ground_truth) return fail(c, PPCR_ERR_INVALID, "ground truth and source clouds differ in size");
        }
        R0 = quat_to_rot(q0);
        resume_forecasts();
        for (double &v : c->dbg_host) v = 0;
        const bool unbounded = (c->max_nb <= 0 || (int64_t)c->max_nb >= c->nt);
        pipelined = c->opt_run_ahead && !unbounded && c->max_nb <= kEllMaxWidth && c->ns > 0;
        max_steps = std::max(inner_steps, 1);
        n_dev_steps = (pipelined && c->nt > 0) ? std::min(max_steps - 1, c->opt_inner_dev_steps) : 0;
        if (pipelined) {
            PPCR_TRY(ensure_loop_state(c));
            loop.st = c->d_loop.p;
            loop.f_tol = f_tol;
            loop.max_steps = max_steps;
            loop.first = 1;
            loop.last_dev = n_dev_steps == 0 ? 1 : 0;
        }
        return PPCR_OK;
    }

    // book one finished outer iteration; mse_truth / moved: NaN unless asked for
    void record(const double Tk[12], const double cost[2], int st, double mse_truth, double moved)
    {
        compose(Tk, Tcum, Tcum);  // T_cum <- T_k * T_cum (cc:101-107)
        const int it = rule.iteration;
        if (history) std::memcpy(history + (size_t)it * 12, Tcum, sizeof(Tcum));
        if (costs) {
            costs[2 * it] = cost[0];
            costs[2 * it + 1] = cost[1];
        }
        if (steps) steps[it] = st;
        if (on_iteration) {
            ppcr_iteration_info info;
            info.iteration = it;
            info.inner_steps = st;
            info.cost[0] = cost[0], info.cost[1] = cost[1];
            std::memcpy(info.T_step, Tk, sizeof(info.T_step));
            std::memcpy(info.T_cum, Tcum, sizeof(info.T_cum));
            info.mse_truth = mse_truth;
            info.moved = moved;
            on_iteration(user, &info);
        }
        rule.cost_drop = (cost[0] - cost[1]) / cost[0];  // cc:119
        rule.iteration++;                                // cc:130
    }

    // What the association of iteration k may know about the registration's moves (ppcr_ctx::move_estimate / move_ratio /
    // move_lag: verlet_lists_pay_off): the move of iteration k - kMaxAhead — consumed for sure when k is enqueued, however
    // far ahead of the results this thread happens to be — or, for the call's first kMaxAhead iterations, what the entry
    // knew, one iteration older each time.  BOTH loops go by this (the host-paced one knows more and does not use it), so
    // that they launch the same kernels at the same iterations and stay bit-identical to each other.
    // (k: the iteration within this call; g: within the sequence of calls it continues)
    void latch_move_forecast(int k)
    {
        const int g = base_iteration + k;
        if (g >= kMaxAhead) {
            c->move_estimate = estimate_of[(g - kMaxAhead) % kMailboxRing];
            c->move_ratio = ratio_of[(g - kMaxAhead) % kMailboxRing];
            c->move_lag = kMaxAhead;
        } else if (g > 0) {
            c->move_estimate = estimate_entry;
            c->move_ratio = ratio_entry;
            c->move_lag = g + 1;
        }
        c->move_forecast_pinned = g > 0;  // (the sequence's first association takes a pending host-side move along and learns from it)
    }
    void note_move(int k, const double T[12])
    {
        const int g = base_iteration + k;
        const double now = move_extent(c, T);
        const double before = g > 0 ? estimate_last : estimate_entry;  // (infinite: a fresh source, nothing before)
        estimate_of[g % kMailboxRing] = now;
        ratio_of[g % kMailboxRing] = (std::isfinite(before) && before > 0) ? now / before : std::numeric_limits<double>::quiet_NaN();
        estimate_last = now;
    }
    // a call on a handle whose last align loop's final move is still pending — nothing has touched the source since —
    // continues that loop's sequence of forecasts
    void resume_forecasts()
    {
        base_iteration = 0;
        if (!(c->pending_from_align && c->move_pending && c->al_iterations > 0)) return;
        base_iteration = c->al_iterations;
        for (int k = 0; k < kMailboxRing; k++) estimate_of[k] = c->al_estimate[k], ratio_of[k] = c->al_ratio[k];
        estimate_entry = c->al_entry_estimate, ratio_entry = c->al_entry_ratio, estimate_last = c->al_last;
    }
    void keep_forecasts(int iterations_done)
    {
        for (int k = 0; k < kMailboxRing; k++) c->al_estimate[k] = estimate_of[k], c->al_ratio[k] = ratio_of[k];
        c->al_entry_estimate = estimate_entry, c->al_entry_ratio = ratio_entry, c->al_last = estimate_last;
        c->al_iterations = base_iteration + iterations_done;
    }

    // Device steps enqueued behind the association of iteration k (this call's count).  Every enqueued step is a grid of
    // workgroups that start, look at the loop state and leave when step 1 ended the inner loop — the common case once a
    // registration has settled (three steps of a 200k cloud: 2 400 idle workgroups, 5.8 us of a 44 us iteration).  So:
    // as many as the last two iterations that are consumed for sure took IN ALL — one more than they needed beyond the
    // first; an inner loop that outgrows them is finished by the host (take_over), same numbers.  By iteration index,
    // like the forecasts: the same launches in every run.
    int dev_steps_for(int k) const
    {
        if (n_dev_steps <= 1 || k < kMaxAhead + 1) return n_dev_steps;
        const int recent = std::max(steps_of[(k - kMaxAhead) % kMailboxRing], steps_of[(k - kMaxAhead - 1) % kMailboxRing]);
        return std::max(1, std::min(recent, n_dev_steps));
    }

    int enqueue()
    {
        StepTicket &tk = in_flight[enq % kMailboxRing];
        // (choices that go by hand-over counts use the count of the iteration kMaxAhead back: consumed for sure, however
        //  far ahead of the results this thread happens to be — the same path in every run)
        c->ovf_decide = enq >= kMaxAhead ? handed_over_of[(enq - kMaxAhead) % kMailboxRing] : ~0u;
        c->ovf_decide_pinned = true;
        latch_move_forecast(enq);
        // moves the source by the previous iteration's transform in its prologue and (steady state) leaves this
        // iteration's partial moments at (q0, t0) behind: K23 folded in
        const int rc_assoc = associate_impl(c, &R0, t0, &tk, &loop);
        c->ovf_decide_pinned = false;
        c->move_forecast_pinned = false;
        if (enq == 0 && base_iteration == 0) {  // (a pending host-side move, taken along by this association, has just set them)
            estimate_entry = c->move_estimate;
            ratio_entry = c->move_ratio;
        }
        PPCR_TRY(rc_assoc);
        if (!c->assoc_folded) PPCR_TRY(launch_step(c, R0, t0, tk, c->assoc_fused, &loop));
        PPCR_TRY(launch_inner(c, tk, loop, dev_steps_for(enq)));
        c->move_on_device = true;     // ... and this iteration's transform is the next pending move
        PPCR_TRY(launch_track(c, tk.seq, report_flags));
        if (enq < 8) trace_mark(c, "enqueued");
        verlet_after[enq % kMailboxRing] = c->verlet_ok;
        enq++;
        return PPCR_OK;
    }

    // LoopState::abort is up: the trains of the iterations behind iteration `done` stepped aside.  Wait for their
    // (empty) mailbox slots and take them back, last first.
    int recall_later_trains()
    {
        while (enq > done + 1) {
            StepResult skipped;
            PPCR_TRY(collect_step(c, in_flight[(enq - 1) % kMailboxRing], skipped));
            if (skipped.status != kLaunchSkipped) return fail(c, PPCR_ERR_STATE, "internal: a launch ran past an aborted iteration");
            enq--;
            c->ovf_parity ^= 1;  // its association had claimed the other counter of the pair
            // (... and would have built or used the rows' Verlet lists: they are as the last association that ran left them)
            c->verlet_ok = verlet_after[(enq - 1) % kMailboxRing];
            c->verlet_order_ok = false;  // (the recalled launch filed no dispatch order; its counters are cleared below)
        }
        return PPCR_OK;
    }

    // The device could not finish iteration `done` by itself (kIterationPending): finish its inner loop one IRLS step at
    // a time, as solve_impl does, hand the pose back to the device and redo what follows an iteration.
    int take_over(StepResult &res)
    {
        const unsigned seq = in_flight[done % kMailboxRing].seq;
        PPCR_TRY(recall_later_trains());
        HIP_TRY(c, hipMemsetAsync(&c->d_loop.p->abort, 0, sizeof(unsigned), c->stream));
        if (c->vcount.p) {
            // the Verlet dispatch order starts over: recalled launches filed nothing and cleared nothing, so every counter
            // is cleared here — with it what the last launch that ran had filed: the next one takes its workgroups in order
            HIP_TRY(c, hipMemsetAsync(c->vcount.p + 16, 0, 48 * sizeof(unsigned), c->stream));
            c->verlet_order_ok = false;
        }
        c->move_on_device = false;
        Mat3 R;
        Vec3 t;
        int st = res.steps;
        for (;;) {
            for (int a = 0; a < 3; a++) {
                for (int b = 0; b < 3; b++) R.m[a][b] = res.T[4 * a + b];
                t[a] = res.T[4 * a + 3];
            }
            StepTicket tk;
            const double c_init = res.cost_init;
            PPCR_TRY(launch_step(c, R, t.v, tk));
            PPCR_TRY(collect_step(c, tk, res));
            res.cost_init = c_init;
            st++;
            const double cost_old = 0.5 * res.sums[16];
            if (res.degenerate) res.cost = cost_old;
            if (res.degenerate || st >= max_steps) break;
            if ((cost_old - res.cost) <= std::max(f_tol * cost_old, 1e-14 * 0.5 * (res.sums[17] + res.sums[18]))) break;
        }
        res.steps = st;
        res.status = kIterationDone;
        for (int a = 0; a < 3; a++) {
            for (int b = 0; b < 3; b++) handback.R[3 * a + b] = res.T[4 * a + b];
            handback.t[a] = res.T[4 * a + 3];
            handback.c[a] = 0.0;
        }
        HIP_TRY(c, hipMemcpyAsync(c->d_pose.p, &handback, sizeof(Pose), hipMemcpyHostToDevice, c->stream));
        c->move_on_device = true;
        return launch_track(c, seq, report_flags);
    }

    int consume()
    {
        StepResult res;
        PPCR_TRY(collect_step(c, in_flight[done % kMailboxRing], res));
        const unsigned seq = in_flight[done % kMailboxRing].seq;
        if (res.status == kIterationPending) PPCR_TRY(take_over(res));
        if (res.status != kIterationDone) return fail(c, PPCR_ERR_STATE, "internal: unexpected mailbox status in the align loop");
        const double cost[2] = {res.cost_init, res.cost};
        double mse_truth = std::numeric_limits<double>::quiet_NaN(), moved = mse_truth;
        if (report_flags) PPCR_TRY(collect_report(c, seq, &mse_truth, &moved));
        std::memcpy(T_last, res.T, sizeof(T_last));
        steps_of[done % kMailboxRing] = res.steps;
        note_move(done, res.T);
        record(res.T, cost, res.steps, mse_truth, moved);
        if (done < 8) trace_mark(c, "consumed");
        handed_over_of[done % kMailboxRing] = c->ovf_last;  // (collect_step has just read it from this iteration's mailbox)
        done++;
        // an iteration enqueued ahead was let through on the strength of the idle count: replay its check now
        if (enq > done && ppcr_stop_rule_check(&rule, n_iter, thresh, patience) != PPCR_CONTINUE)
            return fail(c, PPCR_ERR_STATE, "internal: run-ahead broke the stopping rule");
        return PPCR_OK;
    }

    // Pipelined mode: do whatever can be done without waiting; with may_block, wait for the oldest iteration in flight
    // when nothing else is possible.  *progressed tells a scheduler whether to come back soon.
    int advance(bool may_block, bool *progressed)
    {
        if (progressed) *progressed = false;
        if (finished) return PPCR_OK;
        HIP_TRY(c, hipSetDevice(c->device));
        if (enq == done) {  // nothing in flight: the ordinary check
            if (ppcr_stop_rule_check(&rule, n_iter, thresh, patience) != PPCR_CONTINUE) {
                finished = true;
                if (done > 0) {  // the last transform becomes an ordinary host-side pending move
                    c->move_on_device = false;
                    // (the companion has followed every iteration already: track_kernel)
                    PPCR_TRY(apply_transform_impl(c, T_last, /*defer=*/true, /*move_companion=*/false));
                    // (the next association takes this move along; what is known about it: its ratio to the one before)
                    c->move_ratio = ratio_of[(base_iteration + done - 1) % kMailboxRing];
                    c->pending_from_align = true;
                    keep_forecasts(done);
                }
                if (progressed) *progressed = true;
                return PPCR_OK;
            }
            PPCR_TRY(enqueue());
            if (progressed) *progressed = true;
        }
        // Iterations done .. enq - 1 are in flight (a = enq - done of them).  One more may join them when the checks that
        // will be replayed as they arrive cannot stop the loop whatever their costs turn out to be: the cap is not hit
        // (the iteration count will be rule.iteration + a at the check in question), and the idle count — already
        // updated by the check that let iteration `done` through, at worst one higher after every further check — stays
        // within the patience.  Up to kMaxAhead in flight: the host's launch jitter no longer reaches the device.
        while (enq - done < kMaxAhead) {
            const int a = enq - done;
            if (!((rule.iteration + a != n_iter) && !((double)(rule.idle + a - 1) > patience))) break;
            PPCR_TRY(enqueue());
            if (progressed) *progressed = true;
        }
        if (may_block || step_arrived(c, in_flight[done % kMailboxRing])) {
            PPCR_TRY(consume());
            if (progressed) *progressed = true;
        }
        return PPCR_OK;
    }

    // host-paced loop (unbounded or very wide searches, option run_ahead = 0): one blocking step at a time
    int run_host_paced()
    {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        Tracked tr{nullptr, 0, 0};
        if (report_flags & PPCR_REPORT_MOVED) {
            PPCR_TRY(tracked_cloud(c, tr));
            PPCR_TRY(snapshot_tracked(c, tr));
        }
        while (ppcr_stop_rule_check(&rule, n_iter, thresh, patience) == PPCR_CONTINUE) {
            double Tk[12], cost[2];
            int st = 0;
            latch_move_forecast(done);
            const int rc_assoc = associate_impl(c);
            c->move_forecast_pinned = false;
            PPCR_TRY(rc_assoc);
            if (done == 0 && base_iteration == 0) {
                estimate_entry = c->move_estimate;
                ratio_entry = c->move_ratio;
            }
            PPCR_TRY(solve_impl(c, q0, t0, inner_steps, f_tol, Tk, cost, &st));
            PPCR_TRY(apply_transform_impl(c, Tk, /*defer=*/true));  // rides in the next iteration's K1 prologue
            note_move(done, Tk);
            done++;
            double mse_truth = nan, moved = nan;
            if (report_flags) {
                PPCR_TRY(tracked_cloud(c, tr));
                if (report_flags & PPCR_REPORT_TRUTH) PPCR_TRY(mean_distance(c, tr, c->ground_truth.p, &mse_truth));
                if (report_flags & PPCR_REPORT_MOVED) {
                    PPCR_TRY(mean_distance(c, tr, c->previous.p, &moved));
                    PPCR_TRY(snapshot_tracked(c, tr));
                }
            }
            record(Tk, cost, st, mse_truth, moved);
        }
        if (done > 0) {  // (as the loop that runs ahead leaves it: the pending move comes with its ratio)
            c->move_ratio = ratio_of[(base_iteration + done - 1) % kMailboxRing];
            c->pending_from_align = true;
            keep_forecasts(done);
        }
        finished = true;
        return PPCR_OK;
    }

    // the whole call on this thread
    int run()
    {
        if (!pipelined) return run_host_paced();
        while (!finished) PPCR_TRY(advance(true, nullptr));
        return PPCR_OK;
    }

    // After a failure: leave the handle in a defined state (nothing in flight, no device-resident move, no abort flag).
    void abandon()
    {
        if (!c) return;
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        if (c->d_loop.p) (void)hipMemsetAsync(c->d_loop.p, 0, sizeof(LoopState), c->stream);
        if (c->move_on_device) {
            // the transform the device solved last moves the source the ordinary way at its next use
            Pose P;
            if (hipMemcpy(&P, c->d_pose.p, sizeof(Pose), hipMemcpyDeviceToHost) == hipSuccess) {
                for (int a = 0; a < 3; a++) {
                    for (int b = 0; b < 3; b++) c->pending_T[4 * a + b] = P.R[3 * a + b];
                    c->pending_T[4 * a + 3] = P.t[a];
                }
                c->move_pending = true;
            }
            c->move_on_device = false;
        }
        c->dm2_valid = false;
        c->verlet_ok = false;
        c->verlet_order_ok = false;
        if (c->vcount.p) (void)hipMemsetAsync(c->vcount.p + 16, 0, 48 * sizeof(unsigned), c->stream);
        (void)hipStreamSynchronize(c->stream);
        finished = true;
    }

    // Hand the totals over.  The last move stays pending, as after ppcr_iterate: whoever reads the source next (or the
    // association's distances, weights, reports ...) applies it first; a following ppcr_align / ppcr_iterate takes it
    // along in its first K1 and keeps the temporal cut-off — two calls of n and m iterations cost what one call of
    // n + m does.
    int finish(double *T_final, int *n_done)
    {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (report_flags & PPCR_REPORT_MOVED) c->have_previous = false;  // the loop kept no snapshot of its own
        if (T_final) std::memcpy(T_final, Tcum, sizeof(Tcum));  // identity when no iteration ran
        if (n_done) *n_done = rule.iteration;
        return PPCR_OK;
    }
};

AlignJob make_job(ppcr_ctx *c, int n_iter, double cost_drop_thresh, double n_cost_drop_it, const double q0[4], const double t0[3],
                  int inner_steps, double f_tol, double *history, double *costs, int32_t *steps)
{
    AlignJob j;
    j.c = c;
    j.n_iter = n_iter;
    j.thresh = cost_drop_thresh;
    j.patience = n_cost_drop_it;
    j.inner_steps = inner_steps;
    j.f_tol = f_tol;
    std::memcpy(j.q0, q0, sizeof(j.q0));
    std::memcpy(j.t0, t0, sizeof(j.t0));
    j.history = history;
    j.costs = costs;
    j.steps = steps;
    return j;
}

// align() with the per-iteration outputs optional and the last cumulative transform returned separately
int align_impl(ppcr_ctx *c, int n_iter, double cost_drop_thresh, double n_cost_drop_it, const double q0[4],
               const double t0[3], int inner_steps, double f_tol, double *history, double *costs, int32_t *steps,
               double *T_final, int *n_done, ppcr_stop_rule *rule_io = nullptr, int report_flags = 0,
               ppcr_iteration_fn fn = nullptr, void *user = nullptr)
{
    if (!c) return PPCR_ERR_INVALID;
    if (!q0 || !t0) return fail(c, PPCR_ERR_INVALID, "null argument");
    if (report_flags & ~(PPCR_REPORT_TRUTH | PPCR_REPORT_MOVED)) return fail(c, PPCR_ERR_INVALID, "unknown report flag");
    AlignJob job = make_job(c, n_iter, cost_drop_thresh, n_cost_drop_it, q0, t0, inner_steps, f_tol, history, costs, steps);
    job.report_flags = fn ? report_flags : 0;
    job.on_iteration = fn;
    job.user = user;
    if (rule_io) job.rule = *rule_io;
    c->trace.clear();
    trace_mark(c, "enter");
    PPCR_TRY(job.validate());
    trace_mark(c, "validated");
    const int rc = job.run();
    trace_mark(c, "ran", true);
    if (rc != PPCR_OK) {
        const std::string msg = c->err;
        job.abandon();
        c->err = msg;
        return rc;
    }
    if (rule_io) *rule_io = job.rule;
    const int rc_finish = job.finish(T_final, n_done);
    trace_mark(c, "finished", true);
    trace_print(c);
    return rc_finish;
}

}  // namespace

extern "C" {

int ppcr_align(ppcr_ctx *c, int n_iter, double cost_drop_thresh, double n_cost_drop_it, const double q0[4],
               const double t0[3], int inner_steps, double f_tol, double *history, double *costs, int32_t *steps,
               int *n_done)
{
    return align_impl(c, n_iter, cost_drop_thresh, n_cost_drop_it, q0, t0, inner_steps, f_tol, history, costs, steps,
                      nullptr, n_done);
}

int ppcr_align_report(ppcr_ctx *c, int n_iter, double cost_drop_thresh, double n_cost_drop_it, const double q0[4],
                      const double t0[3], int inner_steps, double f_tol, ppcr_stop_rule *rule_io, int report_flags,
                      ppcr_iteration_fn on_iteration, void *user, double T_final[12], int *n_done)
{
    if (c && n_iter < 0 && !(cost_drop_thresh > 0))
        return fail(c, PPCR_ERR_INVALID, "ppcr_align_report: n_iter < 0 (no iteration cap) needs cost_drop_thresh > 0, or the loop never ends");
    return align_impl(c, n_iter, cost_drop_thresh, n_cost_drop_it, q0, t0, inner_steps, f_tol, nullptr, nullptr, nullptr,
                      T_final, n_done, rule_io, report_flags, on_iteration, user);
}

int ppcr_get_source(ppcr_ctx *c, float *xyz, int64_t stride_bytes)
{
    CTX_ENTER(c);
    if (!c->have_src) return fail(c, PPCR_ERR_STATE, "source cloud not set");
    if (stride_bytes < 12 || stride_bytes % 4) return fail(c, PPCR_ERR_INVALID, "stride_bytes must be a multiple of 4 and >= 12");
    PPCR_TRY(flush_pending_move(c));
    if (c->ns == 0) return PPCR_OK;
    if (!xyz) return fail(c, PPCR_ERR_INVALID, "null output");
    std::vector<float4> h((size_t)c->ns);
    HIP_TRY(c, hipMemcpyAsync(h.data(), c->src.p, sizeof(float4) * (size_t)c->ns, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned char *out = reinterpret_cast<unsigned char *>(xyz);
    for (int64_t r = 0; r < c->ns; r++) {
        int o;
        std::memcpy(&o, &h[(size_t)r].w, 4);
        float *p = reinterpret_cast<float *>(out + (size_t)o * (size_t)stride_bytes);
        p[0] = h[(size_t)r].x;
        p[1] = h[(size_t)r].y;
        p[2] = h[(size_t)r].z;
    }
    return PPCR_OK;
}

// diagnostic (tools/exp_stamps.py): out[8] = per-phase cycle totals over all waves of nn_fast_kernel
int ppcr_debug_get_stamps(ppcr_ctx *c, unsigned long long out[8])
{
    CTX_ENTER(c);
    if (!c->d_stamps.p) return fail(c, PPCR_ERR_STATE, "stamps not enabled");
    const size_t nst = c->stamps_wgs * (kBlock / 64) * 8;  // every workgroup of the launch (idle split slots wrote zeros)
    std::vector<unsigned long long> h(nst);
    HIP_TRY(c, hipMemcpyAsync(h.data(), c->d_stamps.p, nst * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < 8; k++) out[k] = 0;
    for (size_t i = 0; i < nst; i++) out[i % 8] += h[i];
    return PPCR_OK;
}

// diagnostic: wall-clock stamps (100 MHz) of the last fold-and-solve: {entry of the solving block, folded, ticket drawn,
// sums read back, solved, published}
int ppcr_debug_get_fold_stamps(ppcr_ctx *c, unsigned long long out[8])
{
    CTX_ENTER(c);
    if (!c->d_fold_dbg.p) return fail(c, PPCR_ERR_STATE, "fold_stamps not enabled");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, c->d_fold_dbg.p, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PPCR_OK;
}

// diagnostic: the raw per-wave stamp records (8 x u64 per wave) of the last STAMPS launch
int ppcr_debug_get_stamps_raw(ppcr_ctx *c, unsigned long long *out, size_t n)
{
    CTX_ENTER(c);
    if (!c->d_stamps.p) return fail(c, PPCR_ERR_STATE, "stamps not enabled");
    if (n > c->d_stamps.cap) return fail(c, PPCR_ERR_INVALID, "more records than the stamp buffer holds");
    HIP_TRY(c, hipMemcpyAsync(out, c->d_stamps.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PPCR_OK;
}

// diagnostic: host-side figures of the last ppcr_align: {mailbox waits, total wait (s), max wait, -, -, -, max reduce
// launch call, workgroups its associations handed over to the cleanup kernel (summed over the iterations)}
int ppcr_debug_get_host_times(ppcr_ctx *c, double out[8])
{
    CTX_ENTER(c);
    for (int k = 0; k < 8; k++) out[k] = c->dbg_host[k];
    return PPCR_OK;
}

// diagnostic: {reach (cells per radius: 1 = one-pass search), first-pass search radius} of the grid in use
int ppcr_debug_get_search(ppcr_ctx *c, double out[2])
{
    CTX_ENTER(c);
    out[0] = c->grid_valid ? (double)c->reach : 0.0;
    out[1] = c->grid_valid ? c->search_radius : 0.0;
    return PPCR_OK;
}

// diagnostic: the multi-level search's cumulative counters since option "level_stats" was set — out[0] = levels, out[1] = base
// level, then per level: cell radius * 1000, and kLevelDbgWords counters {blocks, handed over (shape), handed over (size), short
// rows listed, staged candidates, rows}
int ppcr_debug_get_levels(ppcr_ctx *c, unsigned *out, int capacity)
{
    CTX_ENTER(c);
    if (!out || capacity < 2 + kMaxLevels * (1 + kLevelDbgWords)) return fail(c, PPCR_ERR_INVALID, "ppcr_debug_get_levels: buffer too small");
    std::memset(out, 0, (size_t)capacity * sizeof(unsigned));
    out[0] = (unsigned)c->n_levels, out[1] = (unsigned)c->base_level;
    std::vector<unsigned> raw((size_t)kMaxLevels * kLevelDbgWords, 0u);
    if (c->level_dbg.p) {
        HIP_TRY(c, hipMemcpyAsync(raw.data(), c->level_dbg.p, raw.size() * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    size_t e = 0;
    for (int l = 0; l < c->n_levels && l < kMaxLevels; l++) {
        const double radius = (l == c->base_level) ? c->search_radius : c->extra_levels[e++].radius;
        unsigned *row = out + 2 + (size_t)l * (1 + kLevelDbgWords);
        row[0] = (unsigned)std::lround(radius * 1000.0);
        for (int k = 0; k < kLevelDbgWords; k++) row[1 + k] = raw[(size_t)l * kLevelDbgWords + (size_t)k];
    }
    return PPCR_OK;
}

// diagnostic: rows the first pass of the most recent two-pass association left short (0 for a one-pass search)
int ppcr_debug_get_short_rows(ppcr_ctx *c, unsigned *out)
{
    CTX_ENTER(c);
    *out = 0;
    if (c->d_short.p) {
        HIP_TRY(c, hipMemcpyAsync(out, c->d_short.p + 2, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return PPCR_OK;
}

// diagnostic: the Verlet lists as the last association left them — out[0] = workgroups of the steady-state grid, out[1] =
// workgroups that failed the completeness test and searched again, CUMULATIVE over the handle's life, out[2] = rows,
// out[3] = rows without a usable list (vg2 = 0), out[4] = sum of the rows' list lengths, out[5] = 1 when the next association
// would trust the lists, out[6] = 1 when the last Verlet launch took its workgroups in the order the one before had filed,
// out[7] = Verlet launches so far, out[8] / out[9] = rows rebuilt one by one / workgroups that did so (cumulative),
// out[10 + j], j < 6: workgroups that searched in the (j + 1)-th last Verlet launch alone, out[16 .. 19]: workgroups that
// held 1 / 2-4 / 5-16 / more failing rows (cumulative)
int ppcr_debug_get_verlet(ppcr_ctx *c, long long out[20])
{
    CTX_ENTER(c);
    for (int k = 0; k < 20; k++) out[k] = 0;
    if (!c->vcount.p || !c->vg2.p || c->ns <= 0) return PPCR_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t rows = (size_t)c->ns;
    std::vector<unsigned char> vn(rows);
    std::vector<float> g2(rows);
    unsigned counters[16];
    HIP_TRY(c, hipMemcpy(counters, c->vcount.p, sizeof(counters), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(vn.data(), c->vn.p, rows, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(g2.data(), c->vg2.p, rows * sizeof(float), hipMemcpyDeviceToHost));
    out[0] = (long long)k1_steady_slots(c), out[1] = (long long)counters[0], out[2] = (long long)rows;
    for (size_t r = 0; r < rows; r++) {
        if (!(g2[r] > 0.f)) out[3]++;
        else out[4] += vn[r];
    }
    out[5] = c->verlet_ok ? 1 : 0;
    out[6] = c->verlet_order_used ? 1 : 0;
    out[7] = (long long)c->verlet_launches;
    out[8] = (long long)counters[1], out[9] = (long long)counters[2];
    for (unsigned j = 0; j < 6 && j < c->verlet_launches; j++) out[10 + j] = (long long)counters[4 + (c->verlet_launches - 1u - j) % 8u];
    for (int j = 0; j < 4; j++) out[16 + j] = (long long)counters[12 + j];
    return PPCR_OK;
}

// diagnostic: a raw copy of one of the handle's device buffers as it stands (no pending move applied, sorted order):
// "vl" [16][ns] int, "vn" [ns] u8, "vg2" / "vacc" [ns] float, "src" [ns] float4, "tgt" [nt] float4 (cell-sorted), "dm2" [ns] u32, "nbr" [m][ns] int, "cnt" [ns] int
int ppcr_debug_read_buffer(ppcr_ctx *c, const char *name, void *dst, size_t bytes)
{
    CTX_ENTER(c);
    if (!name || !dst) return fail(c, PPCR_ERR_INVALID, "null argument");
    const void *p = nullptr;
    size_t have = 0;
    const std::string what = name;
    if (what == "vl") p = c->vl.p, have = c->vl.cap * sizeof(int);
    else if (what == "vn") p = c->vn.p, have = c->vn.cap;
    else if (what == "vg2") p = c->vg2.p, have = c->vg2.cap * sizeof(float);
    else if (what == "vacc") p = c->vacc.p, have = c->vacc.cap * sizeof(float);
    else if (what == "src") p = c->src.p, have = c->src.cap * sizeof(float4);
    else if (what == "tgt") p = c->tgt_sorted.p, have = c->tgt_sorted.cap * sizeof(float4);
    else if (what == "dm2") p = c->dm2.p, have = c->dm2.cap * sizeof(unsigned);
    else if (what == "nbr") p = c->nbr.p, have = c->nbr.cap * sizeof(int);
    else if (what == "cnt") p = c->cnt.p, have = c->cnt.cap * sizeof(int);
    else return fail(c, PPCR_ERR_INVALID, "unknown buffer name");
    if (!p || bytes > have) return fail(c, PPCR_ERR_STATE, "buffer absent or smaller than asked for");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost));
    return PPCR_OK;
}

int ppcr_synchronize(ppcr_ctx *c)
{
    CTX_ENTER(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->grid_pending) HIP_TRY(c, hipEventSynchronize(c->aux_done));
    return PPCR_OK;
}

int ppcr_profile_enable(ppcr_ctx *c, int enable)
{
    CTX_ENTER(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->grid_pending) HIP_TRY(c, hipEventSynchronize(c->aux_done));  // (events of an early grid build)
    for (auto &r : c->prof_recs) {
        c->prof_pool.push_back(r.start);
        c->prof_pool.push_back(r.stop);
    }
    c->prof_recs.clear();
    for (int k = 0; k < K_NUM; k++) {
        c->prof_ms[k] = 0;
        c->prof_n[k] = 0;
    }
    c->prof_on = enable != 0;
    return PPCR_OK;
}

int ppcr_profile_get(ppcr_ctx *c, ppcr_kernel_stat *out, int capacity, int *n_out)
{
    CTX_ENTER(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->grid_pending) HIP_TRY(c, hipEventSynchronize(c->aux_done));
    for (auto &r : c->prof_recs) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, r.start, r.stop) == hipSuccess) {
            c->prof_ms[r.id] += ms;
            c->prof_n[r.id] += 1;
        }
        c->prof_pool.push_back(r.start);
        c->prof_pool.push_back(r.stop);
    }
    c->prof_recs.clear();
    int n = 0;
    for (int k = 0; k < K_NUM; k++) {
        if (c->prof_n[k] == 0) continue;
        if (out && n < capacity) {
            std::memset(&out[n], 0, sizeof(out[n]));
            std::snprintf(out[n].name, sizeof(out[n].name), "%s", kKernelNames[k]);
            out[n].launches = c->prof_n[k];
            out[n].total_ms = c->prof_ms[k];
        }
        n++;
    }
    if (n_out) *n_out = n;
    return PPCR_OK;
}

}  // extern "C"
