// Planned path (k_plan_count, k_plan_scan) and context status kernels.
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, in order; not a standalone header.

namespace {

// ------------------------------------------------------------ k_plan
template <int kMode>
__global__ __launch_bounds__(kThreads) void k_plan_count(BatchDesc d, Plan pl)
{
    __shared__ uint64_t wsum[kWavesPerGroup];
    if (plan_empty(pl))
        return;   // no large buffer: nothing reads local[] / group_pref[] of this launch
    // groups of kThreads entries, grid-stride (the grid is capped: a batch of
    // tens of millions of records launches few workgroups when it has no
    // large buffer and every one of them returns above)
    const uint64_t n = entry_count<kMode>(d);
    for (uint64_t grp = blockIdx.x; grp < pl.ngroups; grp += gridDim.x) {
        const uint64_t i = grp * kThreads + threadIdx.x;
        uint64_t c = 0;
        if (i < n) {   // local[] is still written for every i < d.n
            uint64_t S, E;
            buffer_range<kMode>(d, i, S, E);
            c = is_large(E - S) ? chunk_count(S, E, d.cshift) : 0;
        }
        // exclusive scan over the workgroup: in-wave inclusive scan, then waves
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        uint64_t x = c;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint64_t y = __shfl_up(x, s, kWaveSize);
            if (lane >= s)
                x += y;
        }
        if (lane == 63)
            wsum[w] = x;
        __syncthreads();
        uint64_t before = 0;
        for (int j = 0; j < w; j++)
            before += wsum[j];
        if (i < d.n)
            pl.local[i] = before + x - c;
        if (threadIdx.x == kThreads - 1)
            pl.group_pref[grp] = before + x;   // group total, scanned by k_plan_scan
        __syncthreads();   // wsum is reused by the next group
    }
}

__global__ __launch_bounds__(kThreads) void k_plan_scan(Plan pl)
{
    // single workgroup: exclusive scan of ngroups totals in place, [ngroups] = total
    __shared__ uint64_t wsum[kWavesPerGroup];
    __shared__ uint64_t carry_s;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        carry_s = 0;
        // stream-ordered before this launch's k_chunks; atomic so that a
        // sticky bit set concurrently by another stream's launch survives
        atomicAnd(pl.status, ~kStatusRefused);
    }
    if (plan_empty(pl)) {
        if (threadIdx.x == 0)
            pl.group_pref[pl.ngroups] = 0;
        return;
    }
    __syncthreads();
    for (uint64_t base = 0; base < pl.ngroups; base += kThreads) {
        const uint64_t i = base + threadIdx.x;
        const uint64_t c = i < pl.ngroups ? pl.group_pref[i] : 0;
        uint64_t x = c;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint64_t y = __shfl_up(x, s, kWaveSize);
            if (lane >= s)
                x += y;
        }
        if (lane == 63)
            wsum[w] = x;
        __syncthreads();
        uint64_t before = carry_s;
        for (int j = 0; j < w; j++)
            before += wsum[j];
        if (i < pl.ngroups)
            pl.group_pref[i] = before + x - c;
        __syncthreads();
        if (threadIdx.x == kThreads - 1)
            carry_s = before + x;
        __syncthreads();
    }
    if (threadIdx.x == 0)
        pl.group_pref[pl.ngroups] = carry_s;
}

// Test hook (RAMCRC_OPT_TEST_DIRTY_BINS): corrupt the histogram of a binning
// sequence between its count and scatter passes, as a stale histogram would.
__global__ void k_test_dirty_bins(BinTable* bt, uint32_t par, uint32_t bin, uint32_t add)
{
    if (bin < kNB)
        bt->ctr[par].hist[bin] += add;
}

// ramcrc_ctx_check: take the sticky bits (1, 2) atomically; the old word goes
// to status[1] for the host to read.
__global__ void k_status_take(uint32_t* status)
{
    status[1] = atomicAnd(status, ~(kStatusSticky | kStatusBins));
}


}  // namespace
