// Part of the translation unit ppcr_hip.hip: ppcr_batch_run_small — many small pairs, each registered start to finish by one
// workgroup of one launch.  No handle, no grid, no sort: the host packs the clouds, copies them once, launches, copies the
// records back and synchronises once.  Kernel: ppcr_small.hip.h.  small_batch_run is the host side of both small-batch
// calls; ppcr_batch_run_small_grid (ppcr_hip_small_grid.inc) runs it with its own descriptor, scratch and kernel.

// Bytes of one launch's packed clouds plus stored winners: a batch is cut into launches that stay under it (next to the
// scorer's PPCR_SCORE_D2_BYTES).  Tests lower it through the environment variable PPCR_SMALL_BATCH_BYTES, read at every
// call; a cut changes no pair's result.
#ifndef PPCR_SMALL_BATCH_BYTES
#define PPCR_SMALL_BATCH_BYTES (256ll << 20)
#endif

namespace {

int small_stream(int device, hipStream_t *out, std::string *err)
{
    static std::mutex mu;
    static std::vector<hipStream_t> streams;
    std::lock_guard<std::mutex> lock(mu);
    if ((int)streams.size() <= device) streams.resize((size_t)device + 1, nullptr);
    if (!streams[(size_t)device]) {
        const hipError_t e = hipStreamCreateWithFlags(&streams[(size_t)device], hipStreamNonBlocking);
        if (e != hipSuccess) {
            *err = std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e);
            return PPCR_ERR_HIP;
        }
    }
    *out = streams[(size_t)device];
    return PPCR_OK;
}

template <int M>
void small_launch(const SmallArgs &a, unsigned n, hipStream_t stream)
{
    if (a.md.is_normal) small_align_kernel<M, 0><<<n, kBlock, 0, stream>>>(a);
    else if (a.md.vpd_int == 8) small_align_kernel<M, 8><<<n, kBlock, 0, stream>>>(a);
    else small_align_kernel<M, -1><<<n, kBlock, 0, stream>>>(a);
}

// What the two small-batch entry points differ in (small_batch_run below is everything they share): the descriptor of a
// pair, the device scratch a pair needs besides its stored winners, and the launch.  The other route: ppcr_hip_small_grid.inc.
struct SmallBrute {
    typedef SmallPair Desc;
    static constexpr const char *name = "ppcr_batch_run_small", *kernel = "small_align_kernel";
    static SmallPair &base(Desc &d) { return d; }
    static size_t scratch_bytes(int64_t, int64_t) { return 0; }
    static void describe(Desc &, const float *, const float *, double, size_t) {}
    static void launch(SmallArgs &a, const Desc *pairs, void *, unsigned n, hipStream_t stream)
    {
        a.pairs = pairs;
        if (a.m <= 10) small_launch<10>(a, n, stream);
        else small_launch<20>(a, n, stream);
    }
};

// the memory of one call: taken from the pools, given back when the call returns (the stream is idle by then)
struct SmallBlocks {
    int device;
    void *pinned = nullptr, *dev_in = nullptr, *dev_nbr = nullptr, *dev_out = nullptr, *dev_scratch = nullptr;
    explicit SmallBlocks(int d) : device(d) {}
    ~SmallBlocks()
    {
        pinned_pool(device).give(pinned);
        device_pool(device).free(dev_in);
        device_pool(device).free(dev_nbr);
        device_pool(device).free(dev_out);
        device_pool(device).free(dev_scratch);
    }
};

inline size_t small_round(size_t v) { return (v + 255) / 256 * 256; }

template <class Route>
int small_batch_run(const ppcr_pair *pairs, int64_t n_pairs, const ppcr_batch_options *opt, int device_id, double *T_all,
                    int32_t *n_iter_done, double *history, double *costs, int32_t *steps, char *err, int64_t err_capacity)
{
    typedef typename Route::Desc Desc;
    const std::string who = Route::name;
    auto report = [&](int code, const std::string &msg) {
        if (err && err_capacity > 0) std::snprintf(err, (size_t)err_capacity, "%s", msg.c_str());
        return fail(nullptr, code, msg);
    };
    if (err && err_capacity > 0) err[0] = 0;
    if (n_pairs < 0 || !opt) return report(PPCR_ERR_INVALID, who + ": bad argument");
    if (!(opt->radius > 0) || !std::isfinite(opt->radius)) return report(PPCR_ERR_INVALID, who + ": radius must be positive and finite");
    if (opt->max_neighbours <= 0 || opt->max_neighbours > 20)
        return report(PPCR_ERR_INVALID, who + ": 0 < max_neighbours <= 20 (no unbounded search)");
    if (!(opt->dof > 0) || opt->dim <= 0) return report(PPCR_ERR_INVALID, who + ": dof and dim must be > 0");
    if (opt->n_iter < 0) return report(PPCR_ERR_INVALID, who + ": n_iter must be >= 0");
    if (opt->inner_steps < 1 || opt->inner_steps > 100) return report(PPCR_ERR_INVALID, who + ": 1 <= inner_steps <= 100");
    {
        const double *q = opt->q0, qn = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
        if (!(qn > 0) || !std::isfinite(qn))
            return report(PPCR_ERR_INVALID, who + ": initial rotation quaternion has zero or non-finite norm");
    }
    if (n_pairs == 0) return PPCR_OK;
    if (!pairs || !T_all) return report(PPCR_ERR_INVALID, who + ": null pairs/T_all");
    for (int64_t p = 0; p < n_pairs; p++) {
        const ppcr_pair &pr = pairs[p];
        if (pr.n_source < 1 || pr.n_source > PPCR_SMALL_MAX_POINTS || pr.n_target < 1 || pr.n_target > PPCR_SMALL_MAX_POINTS)
            return report(PPCR_ERR_INVALID, "pair " + std::to_string(p) + ": every cloud must hold 1 .. " +
                                                std::to_string(PPCR_SMALL_MAX_POINTS) + " points (larger pairs: ppcr_batch_run)");
        if (!pr.source || !pr.target || pr.source_stride_bytes < 12 || pr.target_stride_bytes < 12)
            return report(PPCR_ERR_INVALID, "pair " + std::to_string(p) + ": null cloud or stride below 12 bytes");
    }
    int visible = 0;
    if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) {
        (void)hipGetLastError();
        return report(PPCR_ERR_NODEVICE, "no HIP device visible: this library has no CPU fallback");
    }
    if (device_id < 0 || device_id >= visible) return report(PPCR_ERR_INVALID, who + ": device id out of range");
#define SMALL_HIP(expr)                                                                                       \
    do {                                                                                                      \
        const hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) {                                                                               \
            if (stream) (void)hipStreamSynchronize(stream); /* nothing in flight when the blocks go back */   \
            return report(e_ == hipErrorOutOfMemory ? PPCR_ERR_NOMEM : PPCR_ERR_HIP,                          \
                          std::string(#expr) + ": " + hipGetErrorString(e_));                                 \
        }                                                                                                     \
    } while (0)
    hipStream_t stream = nullptr;
    SMALL_HIP(hipSetDevice(device_id));
    {
        std::string msg;
        const int rc = small_stream(device_id, &stream, &msg);
        if (rc != PPCR_OK) return report(rc, msg);
    }

    // the launches: consecutive pairs while the packed clouds and the stored winners stay under the cap (one pair at least)
    const int m = opt->max_neighbours, n_iter = opt->n_iter;
    const bool inner = opt->inner_steps > 1;
    long long cap = PPCR_SMALL_BATCH_BYTES;
    if (const char *e = std::getenv("PPCR_SMALL_BATCH_BYTES"))
        if (*e) cap = std::max(1ll, std::atoll(e));
    struct Launch {
        int64_t first, count;
        size_t floats, nbr, in_at;  // packed floats, stored winners (u16), where its input starts in the pinned block
        size_t scratch;             // the route's device scratch in bytes, every pair's share a multiple of 16
    };
    std::vector<Launch> launches;
    size_t in_total = 0, in_max = 0, nbr_max = 0, scratch_max = 0;
    for (int64_t p = 0; p < n_pairs;) {
        Launch l{p, 0, 0, 0, in_total, 0};
        size_t counted = 0;  // the bytes the cap is about: packed clouds, stored winners, scratch as the header states it
        while (p < n_pairs) {
            const size_t f = 3 * (size_t)(pairs[p].n_source + pairs[p].n_target), w = inner ? (size_t)m * (size_t)pairs[p].n_source : 0;
            const size_t x = Route::scratch_bytes(pairs[p].n_source, pairs[p].n_target);
            if (l.count > 0 && (long long)(counted + 4 * f + 2 * w + x) > cap) break;
            counted += 4 * f + 2 * w + x;
            l.floats += f, l.nbr += w, l.scratch += (x + 15) / 16 * 16, l.count++, p++;
        }
        const size_t bytes = small_round((size_t)l.count * sizeof(Desc)) + small_round(4 * l.floats);
        in_total += bytes;
        in_max = std::max(in_max, bytes);
        nbr_max = std::max(nbr_max, l.nbr);
        scratch_max = std::max(scratch_max, l.scratch);
        launches.push_back(l);
    }
    // the records of the whole batch, one block: T, history, costs (f64), then steps, n_iter_done (i32)
    const size_t np = (size_t)n_pairs, rows = np * (size_t)n_iter;
    const size_t o_T = 0, o_hist = o_T + np * 12, o_cost = o_hist + (history ? rows * 12 : 0), n_f64 = o_cost + (costs ? rows * 2 : 0);
    const size_t o_steps = 0, o_done = o_steps + (steps ? rows : 0), n_i32 = o_done + np;
    const size_t out_bytes = small_round(n_f64 * 8) + small_round(n_i32 * 4);

    SmallBlocks mem(device_id);
    SMALL_HIP(pinned_pool(device_id).take(in_total + out_bytes, &mem.pinned));
    SMALL_HIP(device_pool(device_id).alloc(in_max, &mem.dev_in));
    if (inner) SMALL_HIP(device_pool(device_id).alloc(nbr_max * 2, &mem.dev_nbr));
    SMALL_HIP(device_pool(device_id).alloc(out_bytes, &mem.dev_out));
    if (scratch_max > 0) SMALL_HIP(device_pool(device_id).alloc(scratch_max, &mem.dev_scratch));
    char *const h_in = static_cast<char *>(mem.pinned), *const h_out = h_in + in_total;
    double *const d_f64 = static_cast<double *>(mem.dev_out);
    int *const d_i32 = reinterpret_cast<int *>(static_cast<char *>(mem.dev_out) + small_round(n_f64 * 8));

    SmallArgs a;
    std::memset(&a, 0, sizeof(a));
    a.nbr = static_cast<unsigned short *>(mem.dev_nbr);
    a.T_out = d_f64 + o_T;
    a.history = history ? d_f64 + o_hist : nullptr;
    a.costs = costs ? d_f64 + o_cost : nullptr;
    a.steps = steps ? d_i32 + o_steps : nullptr;
    a.done_out = d_i32 + o_done;
    a.r2 = (float)(opt->radius * opt->radius);
    a.m = m, a.n_iter = n_iter, a.inner_steps = opt->inner_steps;
    a.f_tol = opt->f_tol, a.thresh = opt->cost_drop_thresh, a.patience = opt->n_cost_drop_it;
    {
        const Mat3 R0 = quat_to_rot(opt->q0);
        for (int r = 0; r < 3; r++) {
            for (int k = 0; k < 3; k++) a.R0[3 * r + k] = R0.m[r][k];
            a.t0[r] = opt->t0[r];
        }
    }
    a.md.is_normal = !(opt->dof < std::numeric_limits<double>::infinity());
    a.md.v = opt->dof;
    a.md.texp = -(opt->dof + opt->dim) / 2.0;
    a.md.vpd = opt->dof + opt->dim;
    a.md.vpd_int = 0;
    if (!a.md.is_normal && a.md.vpd == std::floor(a.md.vpd) && a.md.vpd >= 1 && a.md.vpd <= 64) a.md.vpd_int = (int)a.md.vpd;

    hipEvent_t ev[2] = {nullptr, nullptr};
    if (g_trace)
        for (hipEvent_t &e : ev) SMALL_HIP(hipEventCreate(&e));
    float kernel_ms = 0;
    for (size_t li = 0; li < launches.size(); li++) {
        const Launch &l = launches[li];
        // pack: the descriptors, then every pair's source and target as xyz, honouring the strides; the box of the target on the way
        Desc *const desc = reinterpret_cast<Desc *>(h_in + l.in_at);
        const size_t desc_bytes = small_round((size_t)l.count * sizeof(Desc));
        float *const fl = reinterpret_cast<float *>(h_in + l.in_at + desc_bytes);
        size_t at = 0, nbr_at = 0, scratch_at = 0;
        for (int64_t k = 0; k < l.count; k++) {
            const ppcr_pair &pr = pairs[l.first + k];
            SmallPair &d = Route::base(desc[k]);
            d.ns = (int)pr.n_source, d.nt = (int)pr.n_target;
            d.src_off = at;
            const char *s = reinterpret_cast<const char *>(pr.source);
            for (int64_t i = 0; i < pr.n_source; i++, at += 3) std::memcpy(fl + at, s + i * pr.source_stride_bytes, 12);
            d.tgt_off = at;
            const char *t = reinterpret_cast<const char *>(pr.target);
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int64_t i = 0; i < pr.n_target; i++, at += 3) {
                std::memcpy(fl + at, t + i * pr.target_stride_bytes, 12);
                for (int x = 0; x < 3; x++) {
                    lo[x] = std::min(lo[x], fl[at + x]);
                    hi[x] = std::max(hi[x], fl[at + x]);
                }
            }
            for (int x = 0; x < 3; x++) d.c[x] = 0.5 * ((double)lo[x] + (double)hi[x]);
            d.nbr_off = nbr_at;
            if (inner) nbr_at += (size_t)m * (size_t)pr.n_source;
            Route::describe(desc[k], lo, hi, opt->radius, scratch_at);
            scratch_at += (Route::scratch_bytes(pr.n_source, pr.n_target) + 15) / 16 * 16;
        }
        const size_t bytes = desc_bytes + small_round(4 * l.floats);
        SMALL_HIP(hipMemcpyAsync(mem.dev_in, h_in + l.in_at, bytes, hipMemcpyHostToDevice, stream));
        a.packed = reinterpret_cast<float *>(static_cast<char *>(mem.dev_in) + desc_bytes);
        a.first = l.first;
        if (g_trace) SMALL_HIP(hipEventRecord(ev[0], stream));
        Route::launch(a, static_cast<const Desc *>(mem.dev_in), mem.dev_scratch, (unsigned)l.count, stream);
        SMALL_HIP(hipGetLastError());
        if (g_trace) {  // (diagnostic runs only: a synchronisation per launch)
            SMALL_HIP(hipEventRecord(ev[1], stream));
            SMALL_HIP(hipEventSynchronize(ev[1]));
            float ms = 0;
            SMALL_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
            kernel_ms += ms;
        }
    }
    SMALL_HIP(hipMemcpyAsync(h_out, mem.dev_out, out_bytes, hipMemcpyDeviceToHost, stream));
    SMALL_HIP(hipStreamSynchronize(stream));
#undef SMALL_HIP
    if (g_trace) {
        std::fprintf(stderr, "PPCR_TRACE %s pairs=%lld launches=%zu device_ms=%.3f\n", Route::kernel, (long long)n_pairs, launches.size(), kernel_ms);
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }

    const double *const h_f64 = reinterpret_cast<const double *>(h_out);
    const int *const h_i32 = reinterpret_cast<const int *>(h_out + small_round(n_f64 * 8));
    std::memcpy(T_all, h_f64 + o_T, np * 12 * sizeof(double));
    for (size_t p = 0; p < np; p++) {
        const size_t done = (size_t)h_i32[o_done + p], at = p * (size_t)n_iter;
        if (n_iter_done) n_iter_done[p] = (int32_t)done;
        if (history) std::memcpy(history + at * 12, h_f64 + o_hist + at * 12, done * 12 * sizeof(double));
        if (costs) std::memcpy(costs + at * 2, h_f64 + o_cost + at * 2, done * 2 * sizeof(double));
        if (steps) std::memcpy(steps + at, h_i32 + o_steps + at, done * sizeof(int32_t));
    }
    return PPCR_OK;
}

}  // namespace

extern "C" {

int ppcr_batch_run_small(const ppcr_pair *pairs, int64_t n_pairs, const ppcr_batch_options *opt, int device_id, double *T_all,
                         int32_t *n_iter_done, double *history, double *costs, int32_t *steps, char *err, int64_t err_capacity)
{
    return small_batch_run<SmallBrute>(pairs, n_pairs, opt, device_id, T_all, n_iter_done, history, costs, steps, err, err_capacity);
}

}  // extern "C"
