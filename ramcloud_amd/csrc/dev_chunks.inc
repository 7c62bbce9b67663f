// k_chunks (the 8 MiB segment byte scan) and k_combine (per-buffer merge).
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, in order; not a standalone header.

namespace {

// ------------------------------------------------------------ k_chunks
// Scan one chunk [lo, hi) of buffer [S, E) as 1 KiB blocks; returns (in every
// lane) raw(0, zero-padded chunk) relative to the chunk's 1 KiB-aligned end.
__device__ __forceinline__ uint32_t scan_chunk(const uint8_t* lds, const RepOp& op, int lane,
                                               uint64_t S, uint64_t E, uint32_t init,
                                               uint64_t lo, uint64_t hi)
{
    uint32_t u0 = 0, u1 = 0, u2 = 0, u3 = 0;
    uint64_t first = lo & ~uint64_t(kBlock - 1);
    const uint64_t end = (hi + kBlock - 1) & ~uint64_t(kBlock - 1);

    auto step = [&](const u32x4& w) {
        u0 = op.apply(lds, u0, w.x);
        u1 = op.apply(lds, u1, w.y);
        u2 = op.apply(lds, u2, w.z);
        u3 = op.apply(lds, u3, w.w);
    };
    auto special = [&](uint64_t blk) {
        const uint64_t a = blk + uint64_t(lane) * 16;
        u32x4 w = {0u, 0u, 0u, 0u};
        if (a < E && a + 16 > S)
            w = load16(a);
        w.x = fix_word(w.x, a + 0, S, E, init);
        w.y = fix_word(w.y, a + 4, S, E, init);
        w.z = fix_word(w.z, a + 8, S, E, init);
        w.w = fix_word(w.w, a + 12, S, E, init);
        step(w);
    };

    // Head blocks that hold bytes before S or the injected init (S..S+3),
    // and any block cut by E.
    while (first < end && (first < S + 4 || first + kBlock > E)) {
        special(first);
        first += kBlock;
    }
    uint64_t fast_end = end;
    if (first < end && end > E)
        fast_end = end - kBlock;

    // Full blocks: two register groups of kUnroll blocks ping-pong so that one
    // group is always in flight while the other is hashed.  Loads past the
    // range are clamped to the last block (a harmless cached re-read).
    const uint64_t nf = (fast_end - first) / kBlock;
    if (nf > 0) {
        // Buffer loads: the chunk base lives in an SGPR descriptor and the
        // block offset in soffset, so each load costs no address VGPRs.
        const uint32_t lo_w = __builtin_amdgcn_readfirstlane(uint32_t(first));
        const uint32_t hi_w = __builtin_amdgcn_readfirstlane(uint32_t(first >> 32));
        const uint32_t nrec = __builtin_amdgcn_readfirstlane(uint32_t(nf * kBlock));
        void* basep = reinterpret_cast<void*>((uint64_t(hi_w) << 32) | lo_w);
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(basep, (short)0, int(nrec), 0x00020000);
        const uint32_t voff = uint32_t(lane) * 16;
        auto ldb = [&](uint64_t b) -> u32x4 {
            b = b < nf ? b : nf - 1;
            return __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, uint32_t(b * kBlock),
                                                         2 /* nt */);
        };
        u32x4 A[kUnroll], B[kUnroll];
#pragma unroll
        for (int j = 0; j < kUnroll; j++)
            A[j] = ldb(j);
        uint64_t i = 0;
        for (; i + 2 * kUnroll <= nf; i += 2 * kUnroll) {
#pragma unroll
            for (int j = 0; j < kUnroll; j++)
                B[j] = ldb(i + kUnroll + j);
            // keep the whole group's loads issued ahead of the hashing (the
            // scheduler would otherwise sink them next to their uses)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < kUnroll; j++)
                step(A[j]);
#pragma unroll
            for (int j = 0; j < kUnroll; j++)
                A[j] = ldb(i + 2 * kUnroll + j);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < kUnroll; j++)
                step(B[j]);
        }
        // fewer than 2*kUnroll blocks left; A holds blocks i .. i+kUnroll-1
#pragma unroll
        for (int j = 0; j < kUnroll; j++)
            if (i + j < nf)
                step(A[j]);
        if (i + kUnroll < nf) {
#pragma unroll
            for (int j = 0; j < kUnroll; j++)
                B[j] = ldb(i + kUnroll + j);
#pragma unroll
            for (int j = 0; j < kUnroll; j++)
                if (i + kUnroll + j < nf)
                    step(B[j]);
        }
    }
    if (fast_end < end)
        special(fast_end);

    // Fold: in-lane with X^4, then across lanes with X^16 .. X^512.
    uint32_t y = plain_apply(lds, kCombOff, u0) ^ u1;
    y = plain_apply(lds, kCombOff, y) ^ u2;
    y = plain_apply(lds, kCombOff, y) ^ u3;
    uint32_t z = plain_apply(lds, kCombOff, y);
#pragma unroll
    for (int lvl = 0; lvl < 6; lvl++) {
        const uint32_t other = __shfl_xor(z, 1 << lvl, kWaveSize);
        const bool upper = (lane >> lvl) & 1;
        const uint32_t lower_v = upper ? other : z;
        const uint32_t upper_v = upper ? z : other;
        z = plain_apply(lds, kCombOff + (1 + lvl) * 4096, lower_v) ^ upper_v;
    }
    return z;
}

// A record k_obj_compare has work for: a checked type that is not a readable
// object below the large-buffer split (those are compared beside the scan).
__device__ __forceinline__ bool replay_other(const u32x4& r)
{
    const uint32_t type = r.w & 0x3f;
    const uint32_t hdr = replay_header_bytes(type);
    const bool readable = r.z >= hdr && !(r.w & kRecOverlong);
    return hdr != 0 && !(type == RAMCRC_LOG_ENTRY_TYPE_OBJ && readable && !is_large(uint64_t(r.z) - 4));
}



// Locate (entry, chunk) for global chunk index g in general mode.
__device__ __forceinline__ void plan_locate(const Plan& pl, uint64_t n, uint64_t g, uint64_t& entry,
                                            uint64_t& k)
{
    // group: last b with group_pref[b] <= g
    uint64_t lo = 0, hi = pl.ngroups;   // invariant: group_pref[lo] <= g < group_pref[hi]
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (pl.group_pref[mid] <= g) lo = mid; else hi = mid;
    }
    const uint64_t gbase = pl.group_pref[lo];
    uint64_t a = lo * kThreads, b = a + kThreads;
    if (b > n) b = n;
    // last entry j in [a, b) with gbase + local[j] <= g
    uint64_t l2 = a, h2 = b;
    while (h2 - l2 > 1) {
        const uint64_t mid = (l2 + h2) >> 1;
        if (gbase + pl.local[mid] <= g) l2 = mid; else h2 = mid;
    }
    entry = l2;
    k = g - gbase - pl.local[l2];
}

template <int kMode>
__global__ __launch_bounds__(kThreads, 1) void k_chunks(BatchDesc d, Plan pl, uint64_t per_seg)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsChunks];
    if (kMode != kSegAligned && plan_empty(pl))
        return;   // no buffer of this batch is large: skip the table fill too
    fill_replicated(lds, g_tab.stride_large);
    fill_plain(lds, kCombOff, &g_tab.comb[0].t[0][0], 7 * 1024);
    __syncthreads();

    const int lane = threadIdx.x & (kWaveSize - 1);
    const RepOp op(lane);
    const uint64_t wave = uint64_t(blockIdx.x) * kWavesPerGroup +
                          __builtin_amdgcn_readfirstlane(threadIdx.x / kWaveSize);
    const uint64_t nwaves = uint64_t(gridDim.x) * kWavesPerGroup;
    const uint64_t total = kMode == kSegAligned ? per_seg * d.n : pl.group_pref[pl.ngroups];
    if (total > pl.partials_cap) {
        if (wave == 0 && lane == 0)
            atomicOr(pl.status, 3u);   // refused: this launch, and sticky until checked
        return;
    }
    // Work: chunk g -> (buffer i, chunk k), grid stride.
    uint64_t g = wave;
    while (g < total) {
        const uint64_t gnext = g + nwaves;
        uint64_t i, k;
        if (kMode == kSegAligned) {
            i = g / per_seg;
            k = g - i * per_seg;
        } else {
            plan_locate(pl, d.n, g, i, k);
        }
        uint64_t S, E;
        buffer_range<kMode>(d, i, S, E);
        const uint32_t init = d.init ? d.init[i] : 0xFFFFFFFFu;
        const uint64_t cs = S >> d.cshift;
        const uint64_t c_lo = (cs + k) << d.cshift;
        const uint64_t lo = c_lo > S ? c_lo : S;
        const uint64_t c_hi = c_lo + (1ull << d.cshift);
        const uint64_t hi = c_hi < E ? c_hi : E;
        const uint32_t r = scan_chunk(lds, op, lane, S, E, init, lo, hi);
        if (lane == 0)
            pl.partials[g] = r;
        g = gnext;
    }
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src)
{
    const uint32_t lo = __shfl(uint32_t(v), src, kWaveSize);
    const uint32_t hi = __shfl(uint32_t(v >> 32), src, kWaveSize);
    return (uint64_t(hi) << 32) | lo;
}

// ------------------------------------------------------------ k_combine
// Merge the chunk partials of large buffer i (one wave): lane k multiplies
// partial k by x^(8 * 1024 * t), t = its distance to the padded end in 1 KiB
// units; XOR across lanes; x^(-8 pad) removes the padding of the last block.
template <int kMode>
__device__ __forceinline__ void combine_one(const BatchDesc& d, const Plan& pl, uint64_t per_seg,
                                            uint64_t i, uint64_t S, uint64_t E, int lane)
{
    const uint64_t g0 = kMode == kSegAligned ? i * per_seg
                                             : pl.group_pref[i / kThreads] + pl.local[i];
    const uint64_t cnt = chunk_count(S, E, d.cshift);
    const uint64_t cs = S >> d.cshift;
    const uint64_t pend = (E + kBlock - 1) & ~uint64_t(kBlock - 1);
    uint32_t R = 0;
    for (uint64_t k = lane; k < cnt; k += kWaveSize) {
        const uint32_t r = pl.partials[g0 + k];
        const uint64_t ek = (k + 1 == cnt) ? pend : ((cs + k + 1) << d.cshift);
        const uint64_t t = (pend - ek) / kBlock;
        R ^= t ? mulmod_dev(r, xpow_blocks(t)) : r;
    }
#pragma unroll
    for (int lvl = 0; lvl < 6; lvl++)
        R ^= __shfl_xor(R, 1 << lvl, kWaveSize);
    const uint32_t pad = uint32_t(pend - E);
    if (pad)
        R = mulmod_dev(R, g_tab.xinv[pad]);
    if (lane == 0)
        d.out[i] = (d.flags & RAMCRC_FINALIZE) ? ~R : R;
}

// kWide = false: one wave per buffer (few buffers, most of them large).
// kWide = true:  one wave per 64 buffers -- each lane tests one, the wave
// merges the large ones it found -- for big tables of mostly small entries,
// where a wave per entry would cost more than the entries' own scan.
template <int kMode, bool kWide>
__global__ __launch_bounds__(256) void k_combine(BatchDesc d, Plan pl, uint64_t per_seg)
{
    const int lane = threadIdx.x & (kWaveSize - 1);
    const uint64_t wave = uint64_t(blockIdx.x) * (256 / kWaveSize) + threadIdx.x / kWaveSize;
    if (kMode != kSegAligned && (plan_empty(pl) || ((*pl.status) & kStatusRefused)))
        return;   // nothing large, or k_chunks refused the launch (partials overflow)
    const uint64_t n = entry_count<kMode>(d);
    if (!kWide) {
        if (wave >= n)
            return;
        uint64_t S, E;
        buffer_range<kMode>(d, wave, S, E);
        if (is_large(E - S))   // (small ones: k_entries; inactive ones: none)
            combine_one<kMode>(d, pl, per_seg, wave, S, E, lane);
        return;
    }
    if (pl.group_pref[pl.ngroups] == 0)
        return;   // no large buffer in this launch
    // waves of 64 entries, grid-stride (capped grid, as k_plan_count)
    const uint64_t nwave = uint64_t(gridDim.x) * (256 / kWaveSize);
    for (uint64_t wv = wave; wv * kWaveSize < n; wv += nwave) {
        const uint64_t i = wv * kWaveSize + lane;
        uint64_t S = 0, E = 0;
        const bool big = i < n && buffer_range<kMode>(d, i, S, E) && is_large(E - S);
        uint64_t todo = __ballot(big);
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            combine_one<kMode>(d, pl, per_seg, wv * kWaveSize + j, shfl64(S, j), shfl64(E, j), lane);
        }
    }
}


}  // namespace
