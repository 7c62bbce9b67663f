// Host side: HIP error plumbing, the ramcrc_ctx context, launch helpers.
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, in order; not a standalone header.

namespace {

// ------------------------------------------------------------ host side
thread_local int t_last_hip = 0;

#define HIPCHK(expr)                              \
    do {                                          \
        hipError_t e_ = (expr);                   \
        if (e_ != hipSuccess) {                   \
            t_last_hip = int(e_);                 \
            return RAMCRC_EHIP;                   \
        }                                         \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess)
            prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};

}  // namespace

struct ramcrc_ctx {
    int device = 0;
    int ncu = 256;       // CUs the persistent grids are sized for (ramcrc_ctx_set_cus)
    int ncu_all = 256;   // CUs of the device
    std::recursive_mutex mu;   // recursive: the host entry points hold it across their inner device calls
    uint32_t* partials = nullptr;
    uint64_t partials_cap = 0;
    uint64_t* plan_local = nullptr;
    uint64_t plan_cap = 0;
    uint64_t* group_pref = nullptr;
    uint64_t group_cap = 0;
    uint32_t* status = nullptr;
    // small-entry binning
    BinTable* bins = nullptr;
    uint32_t bin_par = 0;   // counter copy of the next binning sequence (BinCounters)
    int fail_after_count = 0;   // RAMCRC_OPT_TEST_FAIL_AFTER_COUNT: abandon N sequences
    uint32_t dirty_bins = 0;    // RAMCRC_OPT_TEST_DIRTY_BINS: bin << 16 | count, once
    int bin_straggler = 0;      // RAMCRC_OPT_TEST_BIN_STRAGGLER: next k_bin_one waits in vain
    int bin_resident[5] = {-1, -1, -1, -1, -1};   // k_bin_one<mode> workgroups per CU (occupancy query)
    // RAMCRC_OPT_BIN_ONE: k_bin_one for batches of <= 1 tile per workgroup; off
    // since round 6, the two-launch binning measured equal or faster
    int bin_one = 0;
    u32x4* sdesc = nullptr;
    uint32_t* sidx = nullptr;
    uint32_t* sinit = nullptr;
    uint64_t sorted_cap = 0;
    // per-object checksums of ramcrc_assemble_objects_device when d_out is NULL
    uint32_t* obj_out = nullptr;
    uint64_t obj_out_cap = 0;
    // ramcrc_segments_certify_device scratch (uint32 words)
    uint32_t* cert_scratch = nullptr;
    uint64_t cert_scratch_cap = 0;
    // host staging for ramcrc_batch_host / ramcrc_stream_host
    uint8_t* h_stage = nullptr;
    uint64_t h_stage_cap = 0;
    uint8_t* d_stage = nullptr;
    uint64_t d_stage_cap = 0;
    hipStream_t copy_stream = nullptr;
    hipStream_t compute_stream = nullptr;
    // parallel segment walk scratch: per part results, per segment flags / bases
    void* walk_parts = nullptr;
    uint64_t walk_parts_cap = 0;
    uint32_t* walk_fallback = nullptr;
    uint64_t walk_fallback_cap = 0;
    uint64_t* walk_base = nullptr;
    uint64_t walk_base_cap = 0;
    void* walk_recs = nullptr;
    uint64_t walk_recs_cap = 0;
    void* walk_pool = nullptr;            // A's records past a part's first 64
    uint64_t walk_pool_cap = 0;
    uint32_t* walk_pool_owner = nullptr;
    uint64_t walk_pool_owner_cap = 0;
    uint32_t* walk_blocks = nullptr;
    uint64_t walk_blocks_cap = 0;
    unsigned long long* walk_pool_used = nullptr;
    uint64_t walk_pool_used_cap = 0;
    int verify_in_walk = 1;         // RAMCRC_OPT_VERIFY_IN_WALK: 0 off, 1 small entries, 2 always
    uint32_t* walk_left = nullptr;  // ramcrc_replay_verify_device, verify-in-walk mode: k_left's list
    uint64_t walk_left_cap = 0;
    uint32_t* walk_sum = nullptr;   // ramcrc_replay_verify_device: the walk's replay_hard summary
    uint64_t walk_sum_cap = 0;
    bool serial_walk = false;   // RAMCRC_OPT_SERIAL_WALK
    uint32_t walk_pshift = 0;   // RAMCRC_OPT_WALK_PART_SHIFT; 0: kPartShift
    // benchmark timing of the scan kernels
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used, ev_free;
};

namespace {

std::atomic<uint64_t> g_scratch_allocations{0};   // ramcrc_debug_scratch_allocations

int grow_device(void** p, uint64_t* cap, uint64_t need_elems, size_t elem)
{
    if (*cap >= need_elems && *p)
        return RAMCRC_OK;
    g_scratch_allocations.fetch_add(1, std::memory_order_relaxed);
    uint64_t n = need_elems < 1024 ? 1024 : need_elems;
    if (*p) {
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipFree(*p));
        *p = nullptr;
        *cap = 0;
    }
    if (hipMalloc(p, n * elem) != hipSuccess) {
        *p = nullptr;
        return RAMCRC_ENOMEM;
    }
    *cap = n;
    return RAMCRC_OK;
}

int reserve_locked(ramcrc_ctx* c, uint64_t max_chunks, uint64_t max_entries)
{
    int rc = grow_device(reinterpret_cast<void**>(&c->partials), &c->partials_cap, max_chunks,
                         sizeof(uint32_t));
    if (rc)
        return rc;
    rc = grow_device(reinterpret_cast<void**>(&c->plan_local), &c->plan_cap, max_entries,
                     sizeof(uint64_t));
    if (rc)
        return rc;
    const uint64_t ngroups = (max_entries + kThreads - 1) / kThreads + 1;
    return grow_device(reinterpret_cast<void**>(&c->group_pref), &c->group_cap, ngroups,
                       sizeof(uint64_t));
}

// Upper bound of chunks for a general batch whose buffers live in device
// memory: every full chunk holds 256 KiB of distinct device bytes, plus at
// most two partial chunks per entry.
// Upper bound of chunks for a general batch whose buffers live in device
// memory: every full chunk holds 256 KiB of distinct device bytes, plus at
// most two partial chunks per entry.  Overlapping or host-mapped buffers can
// exceed it; k_chunks then sets status bit 0 and writes nothing (see
// ramcrc_ctx_reserve).
uint64_t default_chunk_bound(uint64_t n)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess)
        total_b = 288ull << 30;
    return total_b / kChunk + 2 * n + 16;
}

Plan make_plan(ramcrc_ctx* c, uint64_t n)
{
    Plan pl{};
    pl.local = c->plan_local;
    pl.group_pref = c->group_pref;
    pl.ngroups = (n + kThreads - 1) / kThreads;
    pl.partials = c->partials;
    pl.partials_cap = c->partials_cap;
    pl.status = c->status;
    return pl;
}

// Bracket the byte-scan kernel with events when benchmark timing is on.
// Timing-only events: no system-scope fence (cache writeback/invalidate)
// when they are reached, which otherwise puts a ~6 us bubble into the
// stream at every record (two per batch: 16 % of a 1M x 100 B step).  The
// elapsed time is read only after the stream is synchronised.
constexpr unsigned kTimerEventFlags = hipEventDisableSystemFence;

// Times the one launch of its scope.  The two events ride in the kernel's own
// dispatch (hipExtLaunchKernelGGL start/stop events): no separate event
// packets, so no stream bubble before and after the kernel.
struct ScanTimer {
    ramcrc_ctx* c;
    hipStream_t s;
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    ScanTimer(ramcrc_ctx* ctx, hipStream_t stream) : c(ctx), s(stream)
    {
        if (!c->timing)
            return;
        if (!c->ev_free.empty()) {
            ev = c->ev_free.back();
            c->ev_free.pop_back();
        } else if (hipEventCreateWithFlags(&ev.first, kTimerEventFlags) != hipSuccess ||
                   hipEventCreateWithFlags(&ev.second, kTimerEventFlags) != hipSuccess) {
            ev = {nullptr, nullptr};
        }
    }
    template <typename F, typename... Args>
    void launch(F kernel, dim3 grid, dim3 block, Args... args)
    {
        if (ev.first)
            hipExtLaunchKernelGGL(kernel, grid, block, 0, s, ev.first, ev.second, 0, args...);
        else
            hipLaunchKernelGGL(kernel, grid, block, 0, s, args...);
    }
    ~ScanTimer()
    {
        if (ev.first)
            c->ev_used.push_back(ev);
    }
};

int reserve_sorted(ramcrc_ctx* c, uint64_t n)
{
    const uint64_t need = n + uint64_t(kG) * kNB;
    if (c->sorted_cap >= need)
        return RAMCRC_OK;
    uint64_t cap = c->sorted_cap;
    int rc = grow_device(reinterpret_cast<void**>(&c->sdesc), &cap, need, sizeof(u32x4));
    if (rc)
        return rc;
    cap = c->sorted_cap;
    rc = grow_device(reinterpret_cast<void**>(&c->sidx), &cap, need, sizeof(uint32_t));
    if (rc)
        return rc;
    cap = c->sorted_cap;
    rc = grow_device(reinterpret_cast<void**>(&c->sinit), &cap, need, sizeof(uint32_t));
    if (rc)
        return rc;
    c->sorted_cap = cap;
    return RAMCRC_OK;
}

// Small-entry path: bin by step count, scatter into bin order, scan.  A
// binning sequence is k_bin_count (bin_begin) ... k_bin_scatter, k_entries
// (bin_finish), or k_bin_one (bin_begin) ... k_entries for a batch of at most
// one tile per resident workgroup; the planned path runs its chunk kernels in
// between, so that they can exit at once when the count pass found no large
// buffer.
uint64_t bin_grid(const ramcrc_ctx* c, uint64_t n)
{
    // One tile per workgroup up to kBinWgsPerCu workgroups per CU: the binning
    // passes are latency-bound loads of 16 B per entry, and one 4-wave
    // workgroup per CU walking its tiles in turn kept one tile in flight.
    uint64_t grid = (n + uint64_t(kThreads) * kBinPer - 1) / (uint64_t(kThreads) * kBinPer);
    if (grid > uint64_t(c->ncu) * kBinWgsPerCu)
        grid = uint64_t(c->ncu) * kBinWgsPerCu;
    return grid;
}

template <int kMode>
int bin_begin(ramcrc_ctx* c, const BatchDesc& d, hipStream_t s, int skip_large, Sorted* so,
              const uint32_t* sum = nullptr)
{
    if (d.n >= (1ull << 32))
        return RAMCRC_EINVAL;   // sorted slots keep 32-bit entry indices
    int rc = reserve_sorted(c, d.n);
    if (rc)
        return rc;
    *so = Sorted{c->bins, c->sdesc, c->sidx, c->sinit, c->status, c->sorted_cap, c->bin_par, 0};
    // Every launch of this library checks its own error right after it (the
    // timed ScanTimer::launch calls included), so an error pending here was left
    // by a caller's own HIP call on this thread (torch's pointer probes leave
    // such errors behind).  It is recorded for ramcrc_last_hip_error and cleared,
    // not reported as this launch's failure.
    if (hipError_t stale = hipGetLastError(); stale != hipSuccess)
        t_last_hip = int(stale);
    // One launch when one tile per workgroup covers the batch and that grid
    // is resident at once (k_bin_one's arrival count needs every workgroup):
    // at most half the workgroups a CU holds, so that a second context's
    // k_bin_one on another stream fits beside it.  The dirty-histogram test
    // hook needs the two-launch path.
    const uint64_t tiles = (d.n + uint64_t(kThreads) * kBinPer - 1) / (uint64_t(kThreads) * kBinPer);
    int& resident = c->bin_resident[kMode];   // k_bin_one workgroups per CU (under c->mu)
    if (resident < 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_bin_one<kMode>, kThreads, 0) !=
            hipSuccess)
            nb = 0;
        resident = nb;
    }
    if (c->bin_one && !c->dirty_bins && !sum && tiles > 0 &&
        tiles <= uint64_t(c->ncu) * uint64_t(std::min(resident / 2, int(kBinWgsPerCu)))) {
        so->one = 1;
        hipLaunchKernelGGL(k_bin_one<kMode>, dim3(tiles), dim3(kThreads), 0, s, d, *so, skip_large,
                           c->bin_straggler ? 1u : 0u);
        c->bin_straggler = 0;
    } else {
        hipLaunchKernelGGL(k_bin_count<kMode>, dim3(bin_grid(c, d.n)), dim3(kThreads), 0, s, d,
                           *so, skip_large, sum);
    }
    HIPCHK(hipGetLastError());
    // enqueued: it zeroes the other copy, which the next sequence uses
    c->bin_par ^= 1u;
    return RAMCRC_OK;
}

template <int kMode>
int bin_finish(ramcrc_ctx* c, const BatchDesc& d, hipStream_t s, int skip_large, const Sorted& so,
               const uint32_t* sum = nullptr)
{
    if (c->fail_after_count > 0) {   // test hook: a failure after k_bin_count
        c->fail_after_count--;
        return RAMCRC_EHIP;
    }
    if (c->dirty_bins) {   // test hook: a stale histogram
        hipLaunchKernelGGL(k_test_dirty_bins, dim3(1), dim3(1), 0, s, c->bins, so.par,
                           uint32_t(c->dirty_bins >> 16), uint32_t(c->dirty_bins & 0xFFFF));
        c->dirty_bins = 0;
        HIPCHK(hipGetLastError());
    }
    {
        // after k_bin_one: the guarded scatter (exits at once unless k_bin_one aborted)
        hipLaunchKernelGGL(k_bin_scatter<kMode>, dim3(bin_grid(c, d.n)), dim3(kThreads), 0, s, d,
                           so, skip_large, int(so.one), sum);
        HIPCHK(hipGetLastError());
    }
    {
        ScanTimer t(c, s);
        t.launch(k_entries, dim3(c->ncu), dim3(kEntWaves * kWaveSize), d, so);
    }
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

template <int kMode>
int launch_binned(ramcrc_ctx* c, const BatchDesc& d, hipStream_t s, int skip_large)
{
    Sorted so;
    int rc = bin_begin<kMode>(c, d, s, skip_large, &so);
    if (rc)
        return rc;
    return bin_finish<kMode>(c, d, s, skip_large, so);
}

template <int kMode>
int launch_planned(ramcrc_ctx* c, const BatchDesc& d, hipStream_t s, const uint32_t** nother = nullptr,
                   const uint32_t* sum = nullptr)
{
    Sorted so;
    int rc = bin_begin<kMode>(c, d, s, 1, &so, sum);
    if (rc)
        return rc;
    if (nother)
        *nother = &so.bt->ctr[so.par].nother;
    Plan pl = make_plan(c, d.n);
    pl.nlarge = &so.bt->ctr[so.par].nlarge;
    const uint64_t gcap = uint64_t(4) * c->ncu;
    hipLaunchKernelGGL(k_plan_count<kMode>, dim3(uint32_t(pl.ngroups < gcap ? pl.ngroups : gcap)),
                       dim3(kThreads), 0, s, d, pl);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_plan_scan, dim3(1), dim3(kThreads), 0, s, pl);
    HIPCHK(hipGetLastError());
    {
        ScanTimer t(c, s);
        t.launch(k_chunks<kMode>, dim3(c->ncu), dim3(kThreads), d, pl, uint64_t(0));
    }
    HIPCHK(hipGetLastError());
    const uint64_t cw = (d.n + 255) / 256, ccap = uint64_t(16) * c->ncu;
    if (d.n > kWideCombineMin)
        hipLaunchKernelGGL((k_combine<kMode, true>), dim3(uint32_t(cw < ccap ? cw : ccap)), dim3(256), 0, s,
                           d, pl, uint64_t(0));
    else
        hipLaunchKernelGGL((k_combine<kMode, false>), dim3((d.n + 3) / 4), dim3(256), 0, s, d, pl,
                           uint64_t(0));
    HIPCHK(hipGetLastError());
    return bin_finish<kMode>(c, d, s, 1, so, sum);
}


}  // namespace
