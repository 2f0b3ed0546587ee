// Part of the translation unit ppcr_hip.hip: batches of independent pairs (ppcr_align_many, ppcr_batch_run) and the
// pool of handles they keep.

// ---- batches of independent pairs -------------------------------------------------------------------------------
namespace {

// align() on one handle, keeping only the last cumulative transform
int align_final(ppcr_ctx *c, int n_iter, double thresh, double n_cost_drop_it, const double q0[4], const double t0[3],
                int inner_steps, double f_tol, double *T_final, int32_t *n_done)
{
    int done = 0;
    const int rc = align_impl(c, n_iter, thresh, n_cost_drop_it, q0, t0, inner_steps, f_tol, nullptr, nullptr, nullptr,
                              T_final, &done);
    if (rc != PPCR_OK) return rc;
    if (n_done) *n_done = done;
    return PPCR_OK;
}

using sched::FirstError;

}  // namespace

// Handles of ppcr_batch_run, kept between calls: creating one (a stream, the pinned mailbox ring, ~30 device buffers
// that grow on first use) costs ~10 ms, and the allocator serialises the lanes — more than the registrations of a small
// batch themselves (16 pairs of 250k with four in flight: 60 ms with fresh handles every call, 12 ms with pooled ones).
namespace {
struct HandlePool {
    std::mutex mu;
    std::vector<std::pair<int, ppcr_ctx *>> idle;  // (device, handle)
    static constexpr size_t kMaxIdle = 64;
    ppcr_ctx *take(int device)
    {
        std::lock_guard<std::mutex> lk(mu);
        for (size_t k = 0; k < idle.size(); k++)
            if (idle[k].first == device) {
                ppcr_ctx *c = idle[k].second;
                idle.erase(idle.begin() + (long)k);
                return c;
            }
        return nullptr;
    }
    bool give(int device, ppcr_ctx *c)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (idle.size() >= kMaxIdle) return false;
        idle.emplace_back(device, c);
        return true;
    }
    std::vector<ppcr_ctx *> drain()
    {
        std::lock_guard<std::mutex> lk(mu);
        std::vector<ppcr_ctx *> all;
        for (auto &e : idle) all.push_back(e.second);
        idle.clear();
        return all;
    }
};
HandlePool &batch_pool()
{
    static HandlePool *pool = new HandlePool;  // never destroyed: the HIP runtime may be gone by the time statics are
    return *pool;
}
}  // namespace

namespace {

// everything the first association of a registration would wait for, done where waiting costs nothing (the preparing
// thread of ppcr_batch_run): the second half of the grid build, the levels, the source's spatial sort
int prepare_first_association(ppcr_ctx *c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    PPCR_TRY(ensure_grid(c));
    PPCR_TRY(ensure_source_sorted(c));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PPCR_OK;
}

}  // namespace

extern "C" {

int ppcr_align_many(ppcr_ctx *const *ctxs, int n, int lanes, int n_iter, double cost_drop_thresh,
                    double n_cost_drop_it, const double q0[4], const double t0[3], int inner_steps, double f_tol,
                    double *T_final, int32_t *n_done)
{
    if (n < 0 || (n > 0 && (!ctxs || !T_final)) || !q0 || !t0) return PPCR_ERR_INVALID;
    for (int k = 0; k < n; k++) {
        if (!ctxs[k]) return PPCR_ERR_INVALID;
        for (int j = 0; j < k; j++)
            if (ctxs[j] == ctxs[k]) return fail(ctxs[k], PPCR_ERR_INVALID, "ppcr_align_many: the same handle appears twice");
    }
    lanes = std::max(1, std::min(lanes, n));
    // Handles whose loop can run ahead of the host (one inner step per association) are all driven from THIS thread:
    // up to `lanes` of them are in flight at a time, each on its own stream, and the thread only polls their mailboxes
    // — no thread per pair, nothing to oversubscribe when many ranks share few cores.
    {
        std::vector<AlignJob> jobs;
        jobs.reserve((size_t)n);
        bool all_pipelined = true;
        for (int k = 0; k < n && all_pipelined; k++) {
            jobs.push_back(make_job(ctxs[k], n_iter, cost_drop_thresh, n_cost_drop_it, q0, t0, inner_steps, f_tol, nullptr, nullptr, nullptr));
            const int rc = jobs.back().validate();
            if (rc != PPCR_OK) return rc;
            all_pipelined = jobs.back().pipelined;
        }
        if (all_pipelined) {
            int next_job = 0, retired = 0;
            std::vector<int> window;  // indices of the jobs in flight
            while (retired < n) {
                while ((int)window.size() < lanes && next_job < n) window.push_back(next_job++);
                bool any = false;
                for (size_t w = 0; w < window.size();) {
                    AlignJob &j = jobs[(size_t)window[w]];
                    bool progressed = false;
                    const int rc = j.advance(false, &progressed);
                    if (rc != PPCR_OK) {
                        // leave every handle of the batch in a defined state (nothing in flight, no device-resident move)
                        const std::string msg = j.c->err;
                        for (AlignJob &other : jobs) other.abandon();
                        j.c->err = msg;
                        return rc;
                    }
                    any = any || progressed;
                    if (j.finished) {
                        // its last move is queued on its own stream; the synchronising tail runs after the loop
                        window.erase(window.begin() + (long)w);
                        retired++;
                    } else {
                        w++;
                    }
                }
                if (!any) std::this_thread::yield();
            }
            for (int k = 0; k < n; k++) {
                int done = 0;
                const int rc = jobs[(size_t)k].finish(T_final + (size_t)k * 12, &done);
                if (rc != PPCR_OK) return rc;
                if (n_done) n_done[k] = done;
            }
            return PPCR_OK;
        }
    }
    std::atomic<int> next{0};
    FirstError first;
    auto worker = [&]() {
        for (;;) {
            const int k = next.fetch_add(1);
            if (k >= n || first.failed()) return;
            const int rc = align_final(ctxs[k], n_iter, cost_drop_thresh, n_cost_drop_it, q0, t0, inner_steps, f_tol,
                                       T_final + (size_t)k * 12, n_done ? n_done + k : nullptr);
            if (rc != PPCR_OK) first.set(rc, ppcr_last_error(ctxs[k]));
        }
    };
    if (lanes == 1) {
        worker();
    } else {
        std::vector<std::thread> pool;
        for (int l = 0; l < lanes; l++) pool.emplace_back(worker);
        for (auto &th : pool) th.join();
    }
    return first.rc;
}

int ppcr_batch_release(void)
{
    for (ppcr_ctx *c : batch_pool().drain()) ppcr_destroy(c);
    return PPCR_OK;
}

int ppcr_memory_stats(int device_id, uint64_t *reserved_bytes, uint64_t *in_use_bytes, uint64_t *driver_allocs)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, PPCR_ERR_NODEVICE, "no HIP device visible: this library has no CPU fallback");
    }
    if (device_id < 0 || device_id >= n) return fail(nullptr, PPCR_ERR_INVALID, "device_id out of range");
    const PoolStats st = device_pool(device_id).stats();
    if (reserved_bytes) *reserved_bytes = st.reserved_bytes;
    if (in_use_bytes) *in_use_bytes = st.in_use_bytes;
    if (driver_allocs) *driver_allocs = st.driver_allocs;
    return PPCR_OK;
}

int ppcr_memory_trim(int device_id)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(nullptr, PPCR_ERR_NODEVICE, "no HIP device visible: this library has no CPU fallback");
    }
    if (device_id < 0 || device_id >= n) return fail(nullptr, PPCR_ERR_INVALID, "device_id out of range");
    HIP_TRY(nullptr, hipSetDevice(device_id));
    (void)device_pool(device_id).trim();
    pinned_pool(device_id).trim();
    return PPCR_OK;
}

int ppcr_batch_run(const ppcr_pair *pairs, int64_t n_pairs, const ppcr_batch_options *opt, const int *device_ids,
                   int n_devices, int lanes_per_device, double *T_all, int32_t *n_iter_done, char *err,
                   int64_t err_capacity)
{
    auto report = [&](int code, const std::string &msg) {
        if (err && err_capacity > 0) std::snprintf(err, (size_t)err_capacity, "%s", msg.c_str());
        return fail(nullptr, code, msg);
    };
    if (err && err_capacity > 0) err[0] = 0;
    if (n_pairs < 0 || !opt || n_devices <= 0 || !device_ids || lanes_per_device <= 0)
        return report(PPCR_ERR_INVALID, "ppcr_batch_run: bad argument");
    if (n_pairs == 0) return PPCR_OK;
    if (!pairs || !T_all) return report(PPCR_ERR_INVALID, "ppcr_batch_run: null pairs/T_all");
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) {
        (void)hipGetLastError();
        return report(PPCR_ERR_NODEVICE, "no HIP device visible: this library has no CPU fallback");
    }
    for (int d = 0; d < n_devices; d++)
        if (device_ids[d] < 0 || device_ids[d] >= visible) return report(PPCR_ERR_INVALID, "ppcr_batch_run: device id out of range");

    // pair p -> device p % n_devices
    FirstError first;
    // Bounded searches with the device-paced loop (every pair of every batch the command line or batch.py builds): TWO
    // threads per device.  One PREPARES pairs — uploads (synchronous PCIe copies), grid build, levels, source sort: all the
    // waiting of a registration — on handles nobody is iterating on; the other only enqueues and polls, up to
    // `lanes_per_device` registrations in flight on their own streams, as ppcr_align_many does.  A thread per lane
    // (what this was: each doing its own uploads between its iterations) reached 1.07 k pairs/s at two lanes and LESS at
    // four (0.96 k; 64 x 250k on one GPU): every copy held up the other lanes' launches.
    bool two_threads = opt->max_neighbours > 0 && opt->max_neighbours <= kEllMaxWidth;
    for (int64_t p = 0; p < n_pairs && two_threads; p++)
        two_threads = pairs[p].n_source > 0 && (int64_t)opt->max_neighbours < pairs[p].n_target;
    // (the threads and queues of a device's share: sched::run_device_share in ppcr_batch_sched.hpp — the same code runs
    //  under ThreadSanitizer with a host stand-in for these operations, tests/cpp/test_sched.cc)
    struct BatchOps {
        using Handle = ppcr_ctx *;
        using Job = AlignJob;
        const ppcr_pair *pairs;
        const ppcr_batch_options *opt;
        int dev, d, n_devices;
        double *T_all;
        int32_t *n_iter_done;
        int64_t pair_of(int64_t k) const { return (int64_t)d + k * n_devices; }  // pair p -> device p % n_devices
        Handle acquire(int *rc, std::string *err)
        {
            ppcr_ctx *c = batch_pool().take(dev);
            *rc = c ? PPCR_OK : ppcr_create(dev, &c);
            if (*rc != PPCR_OK) {
                *err = ppcr_last_error(nullptr);
                return nullptr;
            }
            return c;
        }
        int prepare(Handle c, int64_t k, std::string *err)
        {
            const int64_t p = pair_of(k);
            const ppcr_pair &pr = pairs[p];
            int rc = ppcr_set_params(c, opt->radius, opt->max_neighbours, opt->dof, opt->dim);
            if (rc == PPCR_OK) rc = ppcr_set_target(c, pr.target, pr.n_target, pr.target_stride_bytes);
            if (rc == PPCR_OK) rc = ppcr_set_source(c, pr.source, pr.n_source, pr.source_stride_bytes);
            if (rc == PPCR_OK) rc = prepare_first_association(c);
            if (rc != PPCR_OK) *err = "pair " + std::to_string(p) + ": " + ppcr_last_error(c);
            return rc;
        }
        std::unique_ptr<Job> start(Handle c, int64_t k, int *rc, std::string *err)
        {
            std::unique_ptr<Job> job(new AlignJob(make_job(c, opt->n_iter, opt->cost_drop_thresh, opt->n_cost_drop_it, opt->q0, opt->t0,
                                                           opt->inner_steps, opt->f_tol, nullptr, nullptr, nullptr)));
            *rc = job->validate();
            if (*rc == PPCR_OK && !job->pipelined) *rc = job->run();  // (a handle that does not run ahead: here and now)
            if (*rc != PPCR_OK) *err = "pair " + std::to_string(pair_of(k)) + ": " + ppcr_last_error(c);
            return job;
        }
        int advance(Job &job, int64_t k, bool *progressed, std::string *err)
        {
            const int rc = job.advance(false, progressed);
            if (rc != PPCR_OK) *err = "pair " + std::to_string(pair_of(k)) + ": " + ppcr_last_error(job.c);
            return rc;
        }
        bool finished(const Job &job) const { return job.finished; }
        Handle handle_of(Job &job) const { return job.c; }
        void retire(Job &job, int64_t k)
        {
            const int64_t p = pair_of(k);
            std::memcpy(T_all + (size_t)p * 12, job.Tcum, sizeof(job.Tcum));
            if (n_iter_done) n_iter_done[p] = job.rule.iteration;
        }
        void abandon(Job &job) { job.abandon(); }
        void release(Handle c, bool ok)
        {
            (void)hipSetDevice(dev);
            if (!ok || hipStreamSynchronize(c->stream) != hipSuccess || !batch_pool().give(dev, c)) ppcr_destroy(c);
        }
    };
    auto device_share = [&](int d) {
        BatchOps ops{pairs, opt, device_ids[d], d, n_devices, T_all, n_iter_done};
        sched::run_device_share(ops, (n_pairs - d + n_devices - 1) / n_devices, lanes_per_device, first);
    };
    // everything else (unbounded or very wide searches: the host-paced loop): a thread per lane, each with its own handle
    std::vector<std::atomic<int64_t>> next(n_devices);
    for (auto &a : next) a.store(0);
    auto worker = [&](int d) {
        ppcr_ctx *c = batch_pool().take(device_ids[d]);
        int rc = c ? PPCR_OK : ppcr_create(device_ids[d], &c);
        if (rc != PPCR_OK) {
            first.set(rc, ppcr_last_error(nullptr));
            return;
        }
        for (;;) {
            const int64_t k = next[d].fetch_add(1);
            const int64_t p = (int64_t)d + k * n_devices;
            if (p >= n_pairs || first.failed()) break;
            const ppcr_pair &pr = pairs[p];
            rc = ppcr_set_params(c, opt->radius, opt->max_neighbours, opt->dof, opt->dim);
            if (rc == PPCR_OK) rc = ppcr_set_target(c, pr.target, pr.n_target, pr.target_stride_bytes);
            if (rc == PPCR_OK) rc = ppcr_set_source(c, pr.source, pr.n_source, pr.source_stride_bytes);
            if (rc == PPCR_OK)
                rc = align_final(c, opt->n_iter, opt->cost_drop_thresh, opt->n_cost_drop_it, opt->q0, opt->t0,
                                 opt->inner_steps, opt->f_tol, T_all + (size_t)p * 12,
                                 n_iter_done ? n_iter_done + p : nullptr);
            if (rc != PPCR_OK) {
                first.set(rc, "pair " + std::to_string(p) + ": " + ppcr_last_error(c));
                break;
            }
        }
        if (rc != PPCR_OK || hipStreamSynchronize(c->stream) != hipSuccess || !batch_pool().give(device_ids[d], c)) ppcr_destroy(c);
    };
    std::vector<std::thread> pool;
    for (int d = 0; d < n_devices; d++) {
        if (two_threads) {
            if (d < n_pairs) pool.emplace_back(device_share, d);  // (d >= n_pairs: an empty share)
            continue;
        }
        const int64_t mine = (n_pairs - d + n_devices - 1) / n_devices;
        if (mine <= 0) continue;  // (an empty share: no thread, no handle)
        const int lanes = (int)std::min<int64_t>(lanes_per_device, mine);
        for (int l = 0; l < lanes; l++) pool.emplace_back(worker, d);
    }
    for (auto &th : pool) th.join();
    if (first.rc != PPCR_OK) return report(first.rc, first.text);
    return PPCR_OK;
}

}  // extern "C"
