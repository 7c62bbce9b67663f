// Small-entry configuration and binning: k_bin_count, k_bin_scatter, k_bin_one.
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, in order; not a standalone header.

namespace {

// ------------------------------------------------------------ k_entries
// Small buffers (log entries, objects; src/ObjectManager.cc:659-669).  A
// group of 8 lanes owns one entry and reads it as 128-byte steps (lane l: 16
// bytes at A + 128 k + 16 l, A = S rounded down to 16): groups of 8 lanes
// reading 128 contiguous bytes stream at the full HBM rate on gfx950 (7.05
// TB/s measured, profiles/r01/membench_access_patterns.txt), while one lane
// per entry reaches only 2 TB/s.  Horner with X^128 per step through the
// replicated LDS tables; at the end the four slot accumulators fold with
// X^4, one GF(2) multiply by x^(8 (16 (7-l) - pad)) moves each lane's partial
// to the entry end (pad = zero bytes past E in the last step), and three
// shuffles XOR the group.  Entries are first binned by step count
// (k_bin_*) so the 8 groups of a wave finish together; bins of at most 8
// steps batch several entry octets per load round.
constexpr int kG = 8;                      // lanes per entry group
constexpr uint64_t kStep = kG * 16;        // bytes per group step
constexpr int kNB = 161;                   // step-count bins
#ifndef RAMCRC_SMALLK
#define RAMCRC_SMALLK 4
#endif
#ifndef RAMCRC_ENT_WAVES
#define RAMCRC_ENT_WAVES 16
#endif
constexpr int kEntWaves = RAMCRC_ENT_WAVES;   // k_entries: waves per workgroup (1 per CU)
constexpr int kSmallK = RAMCRC_SMALLK;     // bins 2..kSmallK: octets loaded one ahead
#ifndef RAMCRC_TINY_K
#define RAMCRC_TINY_K 4
#endif
// bins 2 .. kTinyK (entries of 2 .. kTinyK windows, e.g. objects of 129 ..
// ~500 B): the multi-window tiny phase (tiny_run_cf<true>); 1 = off (the short bins)
constexpr int kTinyK = RAMCRC_TINY_K;
static_assert(kTinyK >= 1 && kTinyK <= 7, "tiny windows: E - A (<= 128 kTinyK) fits 10 bits");

// What a walk record {segment, offset, length, header} rules out for the
// verify: bit 0, the direct one-window tiny path (a record k_obj_compare has
// work for, or an object whose bytes [4, length) span more than one 128-byte
// window -- the walk keeps segments 16-byte aligned, so the windows follow
// from the offset alone); bit 1, the direct multi-window path (anything but
// an object of 2 .. kTinyK windows); bit 2, an object of 3 or more windows.
// The fused replay call ORs this over
// every record its walk writes; unless both bits end up set the verify needs
// no binning scatter (ramcrc_replay_verify_device, k_bin_count).
constexpr uint32_t kHardAll = 3u;
// The fused call's verify-in-walk mode (dev_walk.inc, k_walk_copyv): kSumFast
// when the walk checks the objects itself, kHardFull when some record still
// needs the whole-table verify.
constexpr uint32_t kHardFull = 8u;
constexpr uint32_t kSumFast = 16u;
constexpr uint32_t kSumStage8 = 32u;   // ... with k_walk_copyv's 8 KiB stage (denser batches)
__device__ __forceinline__ uint32_t replay_hard(uint32_t pos, uint32_t len, uint32_t hdr)
{
    const u32x4 r = {0u, pos, len, hdr};
    if (replay_other(r))
        return kHardAll;
    if ((hdr & (0x3f | kRecOverlong)) != RAMCRC_LOG_ENTRY_TYPE_OBJ || len < kObjHeaderBytes)
        return 0u;   // nothing to scan
    const uint32_t s16 = (pos + 1 + ((hdr >> 6) & 3) + 1 + 4) & 15;   // S mod 16
    const uint32_t steps = (s16 + (len - 4) + 127) / 128;             // entry_steps
    if (len - 4 < 4 || steps <= 1)
        return 2u;   // one window (or bytewise): the tiny path
    // (bit 2: more than two windows -- the direct multi-window path then
    // takes the general loop instead of the two-window ring)
    return steps <= 2 ? 1u : (steps <= uint32_t(kTinyK) ? 5u : kHardAll | 4u);
}
#ifndef RAMCRC_PU
#define RAMCRC_PU 2   // A/B on the config-3 mix, 1 KiB and 4 KiB entries: 2 < 1, 3, 4, 6, 8
#endif
constexpr int kPU = RAMCRC_PU;             // ping-pong depth (pipelined bins)
constexpr uint32_t kNoIdx = 0xFFFFFFFFu;   // empty slot
#ifndef RAMCRC_SPLIT_KAPPA
#define RAMCRC_SPLIT_KAPPA 256   // a tiny window in long-phase work units, x 1024
#endif
constexpr uint64_t kSplitKappa = RAMCRC_SPLIT_KAPPA;
#ifndef RAMCRC_OCTET_COST
#define RAMCRC_OCTET_COST 4
#endif
constexpr uint64_t kOctetCost = RAMCRC_OCTET_COST;   // per-octet overhead in step units (work split)
#ifndef RAMCRC_AGE_SKEW
#define RAMCRC_AGE_SKEW 140
#endif
#ifndef RAMCRC_AGE_SKEW_REC
#define RAMCRC_AGE_SKEW_REC 80
#endif
// long bins: share of a wave of age rank r (slot / 4) in 1/2000 of an equal
// share: 2000 + skew * (3 - 2 r), i.e. +-21 % at the outer ranks for skew
// 140.  Same-box A/B (profiles/r03/long/ab_skew*.txt): plain batches gain up
// to skew 120-160 (config-3 mix +4 % over 80), replay verify (records mode)
// loses from 120 on (-3 %), so records mode keeps 80.
constexpr int kAgeSkew = RAMCRC_AGE_SKEW, kAgeSkewRec = RAMCRC_AGE_SKEW_REC;
__host__ __device__ constexpr uint64_t age_weight(uint32_t r, int skew)
{
    return uint64_t(2000 + skew * (3 - 2 * int(r)));
}
static_assert(RAMCRC_ENT_WAVES % 4 == 0, "age ranks of four waves");
#ifndef RAMCRC_BIN_PER
#define RAMCRC_BIN_PER 4
#endif
constexpr int kBinPer = RAMCRC_BIN_PER;    // entries per thread per tile (count/scatter)
#ifndef RAMCRC_BIN_SLICES
#define RAMCRC_BIN_SLICES 8   // k_bin_one: histogram copies (workgroup i adds to copy i % 8: its XCD's)
#endif
constexpr int kBinSlices = RAMCRC_BIN_SLICES;
#ifndef RAMCRC_BIN_WGS_PER_CU
#define RAMCRC_BIN_WGS_PER_CU 8
#endif
constexpr uint64_t kBinWgsPerCu = RAMCRC_BIN_WGS_PER_CU;   // binning grid cap per CU

// XOR of the 8 lanes of a lane group (lanes 8g .. 8g + 7), in every lane:
// quad permutes for lane ^ 1 and ^ 2; then every lane of a quad holds the
// quad's XOR, and row_half_mirror (lane i of a half-row reads lane 7 - i)
// brings in the other quad's -- a VALU op, where the ds_swizzle it replaces
// was an LDS-pipe round trip per window.
__device__ __forceinline__ uint32_t group8_xor_all(uint32_t R)
{
    R ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(R), 0xB1, 0xF, 0xF, false));   // lane ^ 1
    R ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(R), 0x4E, 0xF, 0xF, false));   // lane ^ 2
    R ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(R), 0x141, 0xF, 0xF, false));  // row_half_mirror
    return R;
}

constexpr uint32_t kTinyRow0 = 3;            // tiny phase: row of distance m is m + 3
constexpr uint32_t kLdsTiny = 132 * 1024;    // tiny phase: X^m(byte), m = -3..128
static_assert(kLdsTiny <= kLdsEntries, "k_entries' LDS holds the tiny phase's table");

__device__ __forceinline__ void fill_long(uint8_t* lds)
{
    constexpr uint32_t kRepItems = 4 * 256 * 8;   // as fill_replicated
    constexpr uint32_t kPlain = sizeof(DeviceTables::LongTabs) / 16;
    constexpr uint32_t kR = kRepItems / kEntWaves / kWaveSize;   // 8 per thread at 1024 threads
    constexpr uint32_t kP = (kPlain + kEntWaves * kWaveSize - 1) / (kEntWaves * kWaveSize);
    static_assert(kRepItems % (kEntWaves * kWaveSize) == 0, "rep items per thread");
    const OpTable& op = g_tab.stride_small;
    const uint4* src = reinterpret_cast<const uint4*>(&g_tab.lt);
    uint32_t v[kR];
    uint4 w[kP];
#pragma unroll
    for (uint32_t j = 0; j < kR; j++) {
        const uint32_t idx = threadIdx.x + j * blockDim.x;
        v[j] = op.t[idx >> 11][(idx >> 3) & 255];
    }
#pragma unroll
    for (uint32_t j = 0; j < kP; j++) {
        const uint32_t i = threadIdx.x + j * blockDim.x;
        w[j] = src[i < kPlain ? i : 0];
    }
#pragma unroll
    for (uint32_t j = 0; j < kR; j++) {
        const uint32_t idx = threadIdx.x + j * blockDim.x;
        const uint32_t k = idx >> 11, bv = (idx >> 3) & 255, q = idx & 7;
        const uint32_t off = (k >> 1) * 65536 + bv * 256 + (k & 1) * 128 + q * 16;
        *reinterpret_cast<uint4*>(lds + off) = make_uint4(v[j], v[j], v[j], v[j]);
    }
    uint4* dst = reinterpret_cast<uint4*>(lds + kX4Off);
#pragma unroll
    for (uint32_t j = 0; j < kP; j++) {
        const uint32_t i = threadIdx.x + j * blockDim.x;
        if (i < kPlain)
            dst[i] = w[j];
    }
}

// The counters a binning sequence (k_bin_count -> k_bin_scatter -> k_entries)
// accumulates come in two copies selected by the sequence's parity: sequence
// p counts into copy p while its k_bin_count zeroes copy p ^ 1 for the next
// sequence.  The host flips the parity only once k_bin_count is enqueued, so a
// sequence abandoned after that point (a failed later launch) leaves the next
// one a clean copy; nothing depends on a later kernel of the same sequence
// having run.  k_entries re-checks the layout against what the scatter wrote
// (cursor == count for every bin) before it touches a sorted slot.
struct BinCounters {
    uint64_t cursor[kNB];     // scatter cursors, relative to start
    uint32_t hist[kNB];       // entry counts
    uint32_t nlarge;          // large buffers the count pass left to k_chunks (skip_large)
    uint32_t ninact;          // inactive records (records mode: not checked here)
    uint32_t nother;          // records mode: records k_obj_compare has work for (replay_other)
    uint32_t arrive;          // k_bin_one: workgroups past their histogram atomics
    uint32_t flag;            // k_bin_one: 0, then kBinGo (last arrival) or kBinAbort (a stall)
    uint32_t wide;            // fused replay, direct multi-window path: some object of 3 .. kTinyK windows
    uint32_t hs[kBinSlices][kNB];   // k_bin_one: histogram per slice of workgroups
    uint32_t arr[kBinSlices];       // k_bin_one: arrivals per slice
};

constexpr uint32_t kBinGo = 1, kBinAbort = 2;   // BinCounters::flag: k_bin_one's vote

struct BinTable {
    uint64_t start[kNB];      // first sorted slot of the bin (multiple of 8)
    uint64_t count[kNB];      // entries in the bin
    uint64_t items[kNB + 1];  // exclusive prefix of octets * kmax: work units
    uint64_t kcost[kNB];      // steps charged per octet of the bin (its largest step count)
    uint64_t direct_n;        // nonzero: every entry of this kTable batch is tiny; the tiny
                              // phase reads the caller's table in place (nothing scattered)
    uint64_t direct_multi;    // nonzero: every active entry of this records / table batch is an
                              // object of 2 .. kTinyK windows (bin 2 holds them all); the
                              // multi-window tiny phase reads the record table in place
    uint64_t direct_multi_k2; // ... and none spans more than two windows (the two-window ring)
    BinCounters ctr[2];       // per parity; copy p ^ 1 is zeroed by sequence p's k_bin_count
    uint64_t rescues;         // k_bin_one launches that aborted and were binned by the guarded scatter
};

struct Sorted {
    BinTable* bt;
    u32x4* desc;       // {S lo, S hi, E lo, E hi} per sorted slot
    uint32_t* idx;     // original index; kNoIdx for padding slots
    uint32_t* init;    // initial state per sorted slot (when the batch has one)
    uint32_t* status;  // context status word (bit 2: inconsistent bin layout)
    uint64_t cap;      // sorted slots allocated
    uint32_t par;      // counter copy of this sequence
    uint32_t one;      // host: the sequence was binned by k_bin_one (no scatter launch)
};

// First window of an entry in k_entries: its 128-byte line, so that every
// group load is exactly one cache line -- unless the 4 init bytes at S would
// cross into the second window (S within 3 bytes of the line end); then the
// 16-byte piece of S, as everywhere else.
__device__ __forceinline__ uint64_t line_base(uint64_t S)
{
    return (S & (kStep - 1)) > kStep - 4 ? (S & ~uint64_t(15)) : (S & ~uint64_t(kStep - 1));
}

__device__ __forceinline__ uint64_t entry_steps_line(uint64_t S, uint64_t E)
{
    return (E - line_base(S) + kStep - 1) / kStep;
}

__device__ __forceinline__ uint64_t entry_steps(uint64_t S, uint64_t E)
{
    return (E - (S & ~uint64_t(15)) + kStep - 1) / kStep;
}

// Bin 0: n < 4 (bytewise).  Bins 1..32: exactly that many steps.  Above:
// four bins per octave of the step count.
__device__ __forceinline__ int bin_of(uint64_t S, uint64_t E)
{
    if (E - S < 4)
        return 0;
    const uint64_t K = entry_steps(S, E);
    if (K <= 32)
        return int(K);
    const int m = 63 - __builtin_clzll(K);
    return 33 + 4 * (m - 5) + int((K >> (m - 2)) & 3);
}

__device__ __forceinline__ uint64_t bin_kmax(int b)
{
    if (b <= 32)
        return b == 0 ? 1 : uint64_t(b);
    const int m = (b - 33) / 4 + 5, f = (b - 33) % 4;
    return (uint64_t(5 + f) << (m - 2)) - 1;
}

// One LDS atomic per distinct bin of a wave instead of one per lane (log
// entries fall into a handful of bins, so per-lane atomics serialise).
// Returns this lane's rank among the wave's lanes of the same bin; *base_lane
// receives the previous counter value for the lane's bin.
__device__ __forceinline__ uint32_t wave_bin_add(uint32_t* h, int b, bool active, uint32_t& base)
{
    uint64_t todo = __ballot(active);
    const int lane = threadIdx.x & (kWaveSize - 1);
    uint32_t rank = 0;
    base = 0;
    while (todo) {
        const int leader = int(__builtin_ctzll(todo));
        const int lb = __shfl(b, leader, kWaveSize);
        const uint64_t same = __ballot(active && b == lb);
        uint32_t old = 0;
        if (lane == leader)
            old = atomicAdd(&h[lb], uint32_t(__popcll(same)));
        old = __shfl(old, leader, kWaveSize);
        if (active && b == lb) {
            base = old;
            rank = uint32_t(__popcll(same & ((1ull << lane) - 1)));
        }
        todo &= ~same;
    }
    return rank;
}

// The histogram pass.  It counts entries only: an earlier form also kept the
// largest step count of each log-scale bin with an LDS atomicMax issued,
// lane-masked, between the wave_bin_add loops, and on gfx950 that histogram
// came out wrong in about a quarter of the batches that had log-scale bins
// (entries of bin 33 counted under bins 34-40, 0 of 72 batches once either
// the atomicMax or the ds_bpermute-based wave_bin_add was removed,
// tools/diag_plan_skip.py, DESIGN.md section 9).  A phantom entry left a
// bin's octet of padding slots only, whose interior loop bound Kmin - 1 then
// wrapped: the k_entries hang of round 2.  Each log-scale bin's work estimate
// now uses the bin's upper bound (bin_kmax).
// sum (nullable; records mode, ramcrc_replay_verify_device): the walk's
// replay_hard bits.  Bit 0 clear: every record is inactive or a one-window
// object, so the histogram is "all tiny" without reading the table -- the
// scatter then publishes the direct path, which re-checks every record (a
// record that is not tiny refuses the launch), and the plan and compare
// kernels find nothing.  Bit 1 clear: every record is inactive or an object
// of 2 .. kTinyK windows -- "all in bin 2", the direct multi-window path,
// which re-checks the same way.
template <int kMode>
__global__ __launch_bounds__(kThreads) void k_bin_count(BatchDesc d, Sorted so, int skip_large,
                                                        const uint32_t* sum)
{
    __shared__ uint32_t h[kNB];
    __shared__ uint32_t nlarge, ninact, nother;
    BinCounters& ctr = so.bt->ctr[so.par];
    if (blockIdx.x == 0) {
        // the next sequence's counters (see BinCounters)
        BinCounters& nx = so.bt->ctr[so.par ^ 1];
        for (int t = threadIdx.x; t < kNB; t += blockDim.x) {
            nx.cursor[t] = 0;
            nx.hist[t] = 0;
        }
        for (int t = threadIdx.x; t < kBinSlices * kNB; t += blockDim.x)
            nx.hs[t / kNB][t % kNB] = 0;
        for (int t = threadIdx.x; t < kBinSlices; t += blockDim.x)
            nx.arr[t] = 0;
        if (threadIdx.x == 0) {
            nx.nlarge = 0;
            nx.ninact = 0;
            nx.nother = 0;
            nx.wide = 0;
            nx.arrive = 0;
            nx.flag = 0;
        }
    }
    // the fused replay's summary (replay_hard bits over every walk record):
    // no record beyond one window -- all in bin 1, the direct tiny path; none
    // but objects of 2 .. kTinyK windows -- all in bin 2, the direct
    // multi-window path (bin_layout tells them apart by the bin)
    const uint32_t sv = sum ? *sum : 3u;
    if ((sv & kSumFast) && !(sv & kHardFull))
        return;   // verified in the walk (k_walk_copyv, k_left): an empty layout, nothing to scan
    if (!(sv & 1u) || (kTinyK >= 2 && !(sv & 2u))) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            ctr.hist[(sv & 1u) ? 2 : 1] = uint32_t(entry_count<kMode>(d));
            ctr.wide = (sv & 4u) ? 1u : 0u;
        }
        return;
    }
    for (int t = threadIdx.x; t < kNB; t += blockDim.x)
        h[t] = 0;
    if (threadIdx.x == 0) {
        nlarge = 0;
        ninact = 0;
        nother = 0;
    }
    __syncthreads();
    const uint64_t tile = uint64_t(blockDim.x) * kBinPer;
    const uint64_t n = entry_count<kMode>(d);
    // Records (replay batches of up to ~40M): the next tile's records are in
    // flight while this tile's segment status words are read and binned.
    // Order per tile: status loads (their records arrived last tile), then the
    // next tile's record loads, then the wait for the status words only.
    constexpr bool kPf = kMode == kRecords;
    [[maybe_unused]] u32x4 nr[kBinPer];
    if constexpr (kPf) {
#pragma unroll
        for (int q = 0; q < kBinPer; q++) {
            const uint64_t i = uint64_t(blockIdx.x) * tile + uint64_t(q) * blockDim.x + threadIdx.x;
            nr[q] = i < n ? d.rec[i] : u32x4{0u, 0u, 0u, 0u};
        }
    }
    for (uint64_t base = uint64_t(blockIdx.x) * tile; base < n; base += uint64_t(gridDim.x) * tile) {
        uint64_t S[kBinPer], E[kBinPer];
        bool act[kBinPer], oth[kBinPer];
        if constexpr (kPf) {
            u32x4 cur[kBinPer];
            uint32_t st[kBinPer];
#pragma unroll
            for (int q = 0; q < kBinPer; q++) {
                cur[q] = nr[q];
                const uint64_t i = base + uint64_t(q) * blockDim.x + threadIdx.x;
                st[q] = i < n ? d.seg_status[cur[q].x].x : 0u;
            }
            __builtin_amdgcn_sched_barrier(0);
            const uint64_t nb = base + uint64_t(gridDim.x) * tile;
#pragma unroll
            for (int q = 0; q < kBinPer; q++) {
                const uint64_t i = nb + uint64_t(q) * blockDim.x + threadIdx.x;
                nr[q] = i < n ? d.rec[i] : u32x4{0u, 0u, 0u, 0u};
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < kBinPer; q++) {
                const uint64_t i = base + uint64_t(q) * blockDim.x + threadIdx.x;
                S[q] = E[q] = 0;
                act[q] = i < n && record_range_st(d, cur[q], st[q], S[q], E[q]);
                oth[q] = i < n && replay_other(cur[q]);
            }
        } else {
#pragma unroll
        for (int q = 0; q < kBinPer; q++) {   // all loads first
            const uint64_t i = base + uint64_t(q) * blockDim.x + threadIdx.x;
            S[q] = E[q] = 0;
            oth[q] = false;
            if constexpr (kMode == kRecords) {
                // (the record read once: its range and whether k_obj_compare needs it)
                if (i < n) {
                    const u32x4 r = d.rec[i];
                    act[q] = record_range(d, r, S[q], E[q]);
                    oth[q] = replay_other(r);
                } else {
                    act[q] = false;
                }
            } else {
                act[q] = i < n && buffer_range<kMode>(d, i, S[q], E[q]);
            }
        }
        }
        uint32_t big = 0, inact = 0, other = 0;
#pragma unroll
        for (int q = 0; q < kBinPer; q++) {
            const bool large = skip_large && is_large(E[q] - S[q]);
            big += act[q] && large;
            inact += !act[q] && base + uint64_t(q) * blockDim.x + threadIdx.x < n;
            other += oth[q];
            const bool active = act[q] && !large;
            const int b = active ? bin_of(S[q], E[q]) : 0;
            uint32_t unused;
            wave_bin_add(h, b, active, unused);
        }
        if (__ballot(big != 0)) {   // rare: large buffers are few
            if (big)
                atomicAdd(&nlarge, big);
        }
        if (kMode == kRecords && __ballot(inact != 0)) {
            if (inact)
                atomicAdd(&ninact, inact);
        }
        if (kMode == kRecords && __ballot(other != 0)) {
            if (other)
                atomicAdd(&nother, other);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kNB; t += blockDim.x)
        if (h[t])
            atomicAdd(&ctr.hist[t], h[t]);
    if (threadIdx.x == 0 && nlarge)
        atomicAdd(&ctr.nlarge, nlarge);
    if (threadIdx.x == 0 && ninact)
        atomicAdd(&ctr.ninact, ninact);
    if (threadIdx.x == 0 && nother)
        atomicAdd(&ctr.nother, nother);
}

// Bin layout from the histogram, computed by every k_bin_scatter workgroup
// for itself (no separate scan launch): threads 0..255 take one bin each and
// run parallel exclusive scans of the slot counts and of the work units.
// Workgroup 0 also publishes the layout k_entries reads (start, items, kcost)
// and empties the padding slots of each bin's last octet.  Every thread of
// the block calls this (it synchronises).
struct BinScratch {
    uint64_t start[kNB], count[kNB];
    uint64_t wpos[4], witem[4];
    uint32_t direct, multi;
};

// Returns false (uniformly) when the histogram asks for more sorted slots
// than are allocated -- possible only with a corrupted histogram; the layout
// is then published empty, the status bit set, and nothing is scattered.
// direct_n: the table size when the batch may take the direct tiny path
// (kTable mode), else 0.  When every entry of such a batch is tiny (bins 0-1
// hold all of them), the layout is published empty with direct_n set and
// nothing is scattered: k_entries' tiny phase reads the caller's (off, len,
// init) in place, in index order.
// A counter another workgroup of the same launch may have added to
// (k_bin_one): read at the coherence point, not from this XCD's L2.
__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool bin_layout(const Sorted& so, BinScratch& sc, bool publish,
                                          uint64_t direct_n, const uint32_t* hist = nullptr,
                                          uint64_t multi_n = 0)
{
    BinTable* bt = so.bt;
    const BinCounters& ctr = bt->ctr[so.par];
    const int b = threadIdx.x, lane = b & 63, w = b >> 6;
    if (threadIdx.x == 0) {
        const uint64_t inact = ld_agent(&ctr.ninact);
        sc.direct = direct_n && uint64_t(hist ? hist[0] : ld_agent(&ctr.hist[0])) +
                                        (hist ? hist[1] : ld_agent(&ctr.hist[1])) + inact == direct_n;
        // multi_n (records and table batches): every active entry in bin 2
        // -- the direct multi-window path reads the caller's table in place
        sc.multi = !sc.direct && multi_n &&
                   uint64_t(hist ? hist[2] : ld_agent(&ctr.hist[2])) + inact == multi_n;
    }
    __syncthreads();
    const bool direct = sc.direct, multi = sc.multi;
    if (publish && threadIdx.x == 0) {
        bt->direct_n = direct ? direct_n : 0;
        bt->direct_multi = multi ? multi_n : 0;
        bt->direct_multi_k2 = multi && !ld_agent(&ctr.wide);   // bin 2 proper: two windows at most
    }
    uint64_t cnt = 0, kc = 0, ps = 0, is = 0, pos_c = 0, item_c = 0;
    if (b < 256) {
        if (b < kNB) {
            cnt = direct || multi ? 0 : (hist ? hist[b] : ld_agent(&ctr.hist[b]));
            kc = b <= 32 ? uint64_t(b == 0 ? 1 : b) : bin_kmax(b);
        }
        const uint64_t oct = (cnt + kG - 1) / kG;
        pos_c = oct * kG;
        item_c = b > kTinyK && b >= 2 ? oct * (kc + kOctetCost) : 0;   // bins 0..kTinyK: tiny phases
        ps = pos_c;
        is = item_c;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const uint64_t a1 = __shfl_up(ps, s, kWaveSize);
            const uint64_t a2 = __shfl_up(is, s, kWaveSize);
            if (lane >= s) {
                ps += a1;
                is += a2;
            }
        }
        if (lane == 63) {
            sc.wpos[w] = ps;
            sc.witem[w] = is;
        }
    }
    __syncthreads();
    const bool ok = sc.wpos[0] + sc.wpos[1] + sc.wpos[2] + sc.wpos[3] <= so.cap;
    if (b < kNB) {
        uint64_t pb = 0, ib = 0;
        for (int j = 0; j < w; j++) {
            pb += sc.wpos[j];
            ib += sc.witem[j];
        }
        const uint64_t start = ok ? pb + ps - pos_c : 0, items = ok ? ib + is - item_c : 0;
        sc.start[b] = start;
        sc.count[b] = ok ? cnt : 0;
        if (publish) {
            bt->start[b] = start;
            bt->count[b] = ok ? cnt : 0;
            bt->items[b] = items;
            bt->kcost[b] = kc + kOctetCost;
            if (b == kNB - 1)
                bt->items[kNB] = ok ? items + item_c : 0;
        }
    }
    if (!ok) {
        if (publish && threadIdx.x == 0)
            atomicOr(so.status, kStatusSticky | kStatusBins);
        return false;
    }
    __syncthreads();
    if (publish) {
        for (int t = threadIdx.x; t < kNB * kG; t += blockDim.x) {
            const int bb = t / kG, j = t % kG;
            const uint64_t c = sc.count[bb];
            const uint64_t slot = c + uint64_t(j);
            if ((c % kG) && slot < (c + kG - 1) / kG * kG) {
                so.desc[sc.start[bb] + slot] = u32x4{0u, 0u, 0u, 0u};
                so.idx[sc.start[bb] + slot] = kNoIdx;
            }
        }
    }
    return true;
}

// rescue: the guarded scatter after a k_bin_one (see there): nothing to do
// when k_bin_one's vote went kBinGo; otherwise the histogram is the sum of
// k_bin_one's slices, which every workgroup of it added to before it voted.
template <int kMode>
__global__ __launch_bounds__(kThreads) void k_bin_scatter(BatchDesc d, Sorted so, int skip_large,
                                                          int rescue, const uint32_t* sum)
{
    // verified in the walk (kSumFast, no kHardFull): only workgroup 0 has work,
    // publishing the empty layout k_entries reads
    if (sum && blockIdx.x != 0 && (*sum & (kSumFast | kHardFull)) == kSumFast)
        return;
    __shared__ uint32_t cnt[kNB];
    __shared__ uint64_t base[kNB];
    __shared__ BinScratch sc;
    __shared__ uint32_t tot[kNB];
    __shared__ uint32_t vote;
    BinCounters& ctr = so.bt->ctr[so.par];
    if (rescue) {
        // one load per workgroup (k_bin_one has ended: the flag is final); a
        // load per thread put 250K same-address loads on the fabric (5 us)
        if (threadIdx.x == 0)
            vote = ld_agent(&ctr.flag);
        __syncthreads();
        if (vote == kBinGo)
            return;
        for (int t = threadIdx.x; t < kNB; t += blockDim.x) {
            uint32_t all = 0;
#pragma unroll
            for (int j = 0; j < kBinSlices; j++)
                all += ld_agent(&ctr.hs[j][t]);
            tot[t] = all;
            if (blockIdx.x == 0)
                ctr.hist[t] = all;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0)
            atomicAdd(reinterpret_cast<unsigned long long*>(&so.bt->rescues), 1ull);
    }
    for (int t = threadIdx.x; t < kNB; t += blockDim.x)
        cnt[t] = 0;
    __syncthreads();
    if (!bin_layout(so, sc, blockIdx.x == 0,
                    (kMode == kTable || kMode == kRecords) ? entry_count<kMode>(d) : 0,
                    rescue ? tot : nullptr,
                    (kMode == kRecords || kMode == kTable) && kTinyK >= 2
                        ? entry_count<kMode>(d) : 0))
        return;   // corrupted histogram: nothing is scattered, k_entries refuses
    if (sc.direct || sc.multi)
        return;   // all tiny / all of 2 .. kTinyK windows: k_entries reads the table in place
    if (sc.wpos[0] + sc.wpos[1] + sc.wpos[2] + sc.wpos[3] == 0)
        return;   // every bin empty (nothing active, or verified in the walk): nothing to place
    unsigned long long* cursor = reinterpret_cast<unsigned long long*>(ctr.cursor);
    const uint64_t tile = uint64_t(blockDim.x) * kBinPer;
    const uint64_t n = entry_count<kMode>(d);
    for (uint64_t t0 = uint64_t(blockIdx.x) * tile; t0 < n; t0 += uint64_t(gridDim.x) * tile) {
        uint64_t S[kBinPer], E[kBinPer];
        int b[kBinPer];
        uint32_t lp[kBinPer];
        bool act[kBinPer];
#pragma unroll
        for (int q = 0; q < kBinPer; q++) {
            const uint64_t i = t0 + uint64_t(q) * blockDim.x + threadIdx.x;
            S[q] = E[q] = 0;
            act[q] = i < n && buffer_range<kMode>(d, i, S[q], E[q]);
        }
#pragma unroll
        for (int q = 0; q < kBinPer; q++) {
            const bool active = act[q] && !(skip_large && is_large(E[q] - S[q]));
            b[q] = active ? bin_of(S[q], E[q]) : 0;
            uint32_t wbase;
            const uint32_t rank = wave_bin_add(cnt, b[q], active, wbase);
            lp[q] = wbase + rank;
            if (!active)
                b[q] = -1;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < kNB; t += blockDim.x)
            if (cnt[t]) {
                base[t] = atomicAdd(&cursor[t], (unsigned long long)cnt[t]);
                cnt[t] = 0;
            }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kBinPer; q++) {
            // a slot past the bin's count (a histogram that disagrees with
            // this pass) is not written; the cursor still counts it, so
            // k_entries sees cursor != count and refuses the launch
            if (b[q] >= 0 && base[b[q]] + lp[q] < sc.count[b[q]]) {
                const uint64_t i = t0 + uint64_t(q) * blockDim.x + threadIdx.x;
                const uint64_t pos = sc.start[b[q]] + base[b[q]] + lp[q];
                so.desc[pos] = u32x4{uint32_t(S[q]), uint32_t(S[q] >> 32), uint32_t(E[q]),
                                     uint32_t(E[q] >> 32)};
                so.idx[pos] = uint32_t(i);
                if (d.init)
                    so.init[pos] = d.init[i];
            }
        }
        __syncthreads();
    }
}

// One-launch binning for batches of at most one tile per workgroup, with the
// grid expected resident at once (bin_begin checks both): each workgroup loads
// its tile once, ranks every entry inside its bin with the same wave_bin_add
// as the count pass, and takes its range of each bin with one returning
// atomic on the histogram -- the value the two-launch path's scatter cursor
// would give.  After a grid-wide arrival every workgroup lays the bins out
// from the now complete histogram and writes its descriptors from registers.
// Saves the scatter's second read of the table.
//
// The arrival cannot be guaranteed: another context's kernels on another
// stream (a k_entries workgroup takes a whole CU; a second k_bin_one takes
// the other half) or a preempted queue can keep part of the grid from being
// dispatched while the rest waits.  So the wait is a vote, never a
// precondition: the last arrival tries to turn the flag from 0 to kBinGo, a
// waiter that has seen no arrival anywhere in the grid for kBinStallTicks
// tries to turn it from 0 to kBinAbort, and the one compare-and-swap that
// wins decides for every workgroup, including those dispatched later.  On
// abort nothing is scattered; the guarded scatter launched after every
// k_bin_one (k_bin_scatter with `rescue`) exits at once on kBinGo and
// otherwise bins the batch the two-launch way from the histogram k_bin_one
// completed.  A grid that cannot all be resident therefore costs one stall
// period and a second read of the table, never a wrong or refused launch.
#ifndef RAMCRC_BIN_SLEEP
#define RAMCRC_BIN_SLEEP 4   // s_sleep between polls (x 64 cycles)
#endif
#ifndef RAMCRC_BIN_STALL_US
#define RAMCRC_BIN_STALL_US 30   // k_bin_one: abort after this long with no arrival in the grid
#endif
// No fences: on this 8-XCD part an agent-scope release / acquire writes back
// / invalidates the XCD's L2 (per thread), which cost more than the whole
// two-launch binning.  Everything that crosses workgroups here is an atomic
// (the histogram adds, performed before the wave passes s_waitcnt, the
// arrival counts, the flag, and bin_layout's reads of the histogram).
constexpr uint64_t kBinStallTicks = uint64_t(RAMCRC_BIN_STALL_US) * 100;   // 100 MHz clock
__device__ __forceinline__ uint32_t bin_arrivals(const BinCounters& ctr)
{
    uint32_t a = 0;
#pragma unroll
    for (int j = 0; j < kBinSlices; j++)
        a += __hip_atomic_load(&ctr.arr[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return a;
}

__device__ __forceinline__ uint32_t bin_vote(BinCounters& ctr, uint32_t want)
{
    uint32_t expect = 0;
    __hip_atomic_compare_exchange_strong(&ctr.flag, &expect, want, __ATOMIC_RELAXED,
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect ? expect : want;   // the value that won
}

// Two-level arrival: a workgroup counts itself in its slice (workgroups
// i % kBinSlices), the last of a slice counts the slice in `arrive`, the last
// slice votes kBinGo (one counter for the whole grid serialised its ~1,000
// arrivals: ~5 us).  Returns true when kBinGo won the vote.  The clock is the
// 100 MHz s_memrealtime; a stall measured across a preemption only makes the
// abort (the slower, always correct path) more likely.
__device__ __forceinline__ bool grid_arrive(BinCounters& ctr, uint32_t nwg)
{
    __shared__ uint32_t all_in;
    __builtin_amdgcn_s_waitcnt(0);   // this wave's histogram atomics are performed
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t sl = blockIdx.x % kBinSlices;
        const uint32_t in_sl = nwg / kBinSlices + (sl < nwg % kBinSlices ? 1u : 0u);
        const uint32_t nsl = nwg < uint32_t(kBinSlices) ? nwg : uint32_t(kBinSlices);
        bool last = __hip_atomic_fetch_add(&ctr.arr[sl], 1u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT) + 1 == in_sl;
        if (last)
            last = __hip_atomic_fetch_add(&ctr.arrive, 1u, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT) + 1 == nsl;
        uint32_t f;
        if (last) {
            f = bin_vote(ctr, kBinGo);
        } else {
            uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            uint32_t seen = bin_arrivals(ctr);
            while ((f = __hip_atomic_load(&ctr.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0) {
                const uint64_t now = __builtin_amdgcn_s_memrealtime();
                if (now - t0 > kBinStallTicks) {
                    const uint32_t a = bin_arrivals(ctr);
                    if (a == seen) {
                        f = bin_vote(ctr, kBinAbort);   // nobody arrived for a whole period
                        break;
                    }
                    seen = a;
                    t0 = now;
                }
                __builtin_amdgcn_s_sleep(RAMCRC_BIN_SLEEP);
            }
        }
        all_in = f == kBinGo;
    }
    __syncthreads();
    return all_in;
}

template <int kMode>
__global__ __launch_bounds__(kThreads) void k_bin_one(BatchDesc d, Sorted so, int skip_large,
                                                      uint32_t straggler)
{
    __shared__ uint32_t h[kNB];
    __shared__ uint64_t base[kNB];
    __shared__ uint32_t nlarge, ninact, nother;
    __shared__ BinScratch sc;
    BinCounters& ctr = so.bt->ctr[so.par];
    if (blockIdx.x == 0) {
        BinCounters& nx = so.bt->ctr[so.par ^ 1];   // the next sequence's counters
        for (int t = threadIdx.x; t < kNB; t += blockDim.x) {
            nx.cursor[t] = 0;
            nx.hist[t] = 0;
        }
        for (int t = threadIdx.x; t < kBinSlices * kNB; t += blockDim.x)
            nx.hs[t / kNB][t % kNB] = 0;
        for (int t = threadIdx.x; t < kBinSlices; t += blockDim.x)
            nx.arr[t] = 0;
        if (threadIdx.x == 0) {
            nx.nlarge = 0;
            nx.ninact = 0;
            nx.nother = 0;
            nx.wide = 0;
            nx.arrive = 0;
            nx.flag = 0;
        }
    }
    for (int t = threadIdx.x; t < kNB; t += blockDim.x)
        h[t] = 0;
    if (threadIdx.x == 0) {
        nlarge = 0;
        ninact = 0;
        nother = 0;
    }
    __syncthreads();
    const uint64_t n = entry_count<kMode>(d);
    const uint64_t t0 = uint64_t(blockIdx.x) * blockDim.x * kBinPer;
    uint64_t S[kBinPer], E[kBinPer];
    bool act[kBinPer], oth[kBinPer];
    uint32_t in0[kBinPer];
#pragma unroll
    for (int q = 0; q < kBinPer; q++) {   // all loads first
        const uint64_t i = t0 + uint64_t(q) * blockDim.x + threadIdx.x;
        S[q] = E[q] = 0;
        oth[q] = false;
        if constexpr (kMode == kRecords) {
            if (i < n) {
                const u32x4 r = d.rec[i];
                act[q] = record_range(d, r, S[q], E[q]);
                oth[q] = replay_other(r);
            } else {
                act[q] = false;
            }
        } else {
            act[q] = i < n && buffer_range<kMode>(d, i, S[q], E[q]);
        }
        in0[q] = d.init && i < n ? d.init[i] : 0u;
    }
    int b[kBinPer];
    uint32_t lp[kBinPer];
    uint32_t big = 0, inact = 0, other = 0;
#pragma unroll
    for (int q = 0; q < kBinPer; q++) {
        const bool large = skip_large && is_large(E[q] - S[q]);
        big += act[q] && large;
        inact += !act[q] && t0 + uint64_t(q) * blockDim.x + threadIdx.x < n;
        other += oth[q];
        const bool active = act[q] && !large;
        b[q] = active ? bin_of(S[q], E[q]) : 0;
        uint32_t wbase;
        const uint32_t rank = wave_bin_add(h, b[q], active, wbase);
        lp[q] = wbase + rank;
        if (!active)
            b[q] = -1;
    }
    if (__ballot(big != 0) && big)
        atomicAdd(&nlarge, big);
    if (kMode == kRecords && __ballot(inact != 0) && inact)
        atomicAdd(&ninact, inact);
    if (kMode == kRecords && __ballot(other != 0) && other)
        atomicAdd(&nother, other);
    __syncthreads();
    const int sl = int(blockIdx.x % kBinSlices);
    for (int t = threadIdx.x; t < kNB; t += blockDim.x)
        base[t] = h[t] ? atomicAdd(&ctr.hs[sl][t], h[t]) : 0u;
    if (threadIdx.x == 0 && nlarge)
        atomicAdd(&ctr.nlarge, nlarge);
    if (threadIdx.x == 0 && ninact)
        atomicAdd(&ctr.ninact, ninact);
    if (threadIdx.x == 0 && nother)
        atomicAdd(&ctr.nother, nother);
    // (straggler: test hook, one workgroup more than launched, which never comes)
    if (!grid_arrive(ctr, gridDim.x + straggler))
        return;   // aborted: the guarded scatter bins the batch
    constexpr bool kDirect = kMode == kTable || kMode == kRecords;
    if constexpr (kDirect) {
        // Every entry tiny (the direct path: nothing to scatter)?  Bins 0 and
        // 1 and the inactive count decide it -- 17 loads instead of the 8 x 161
        // below -- and then only workgroup 0 has work left: publishing the
        // (empty) layout.
        __shared__ uint32_t all_tiny;
        if (threadIdx.x < 2) {
            uint32_t all = 0;
#pragma unroll
            for (int j = 0; j < kBinSlices; j++)
                all += ld_agent(&ctr.hs[j][threadIdx.x]);
            h[threadIdx.x] = all;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            all_tiny = uint64_t(h[0]) + h[1] + ld_agent(&ctr.ninact) == n;
        __syncthreads();
        if (all_tiny) {
            if (blockIdx.x == 0) {
                if (threadIdx.x < 2)
                    ctr.hist[threadIdx.x] = h[threadIdx.x];
                bin_layout(so, sc, true, n, h);   // direct: reads bins 0 and 1 only
                for (int t = threadIdx.x; t < kNB; t += blockDim.x)
                    ctr.cursor[t] = sc.count[t];
            }
            return;
        }
    }
    // totals, and this workgroup's place behind the earlier slices (reading
    // the slices here beat having the last arrival publish the totals)
    for (int t = threadIdx.x; t < kNB; t += blockDim.x) {
        uint32_t all = 0, before = 0;
#pragma unroll
        for (int j = 0; j < kBinSlices; j++) {
            const uint32_t v = ld_agent(&ctr.hs[j][t]);
            before += j < sl ? v : 0u;
            all += v;
        }
        h[t] = all;
        base[t] += before;
        if (blockIdx.x == 0)
            ctr.hist[t] = all;
    }
    __syncthreads();
    const bool ok = bin_layout(so, sc, blockIdx.x == 0,
                               (kMode == kTable || kMode == kRecords) ? n : 0, h,
                               (kMode == kRecords || kMode == kTable) && kTinyK >= 2 ? n : 0);
    if (blockIdx.x == 0)   // what k_entries checks: every bin holds what was placed in it
        for (int t = threadIdx.x; t < kNB; t += blockDim.x)
            ctr.cursor[t] = sc.count[t];
    if (!ok || sc.direct)
        return;
#pragma unroll
    for (int q = 0; q < kBinPer; q++) {
        if (b[q] >= 0 && base[b[q]] + lp[q] < sc.count[b[q]]) {
            const uint64_t i = t0 + uint64_t(q) * blockDim.x + threadIdx.x;
            const uint64_t pos = sc.start[b[q]] + base[b[q]] + lp[q];
            so.desc[pos] = u32x4{uint32_t(S[q]), uint32_t(S[q] >> 32), uint32_t(E[q]),
                                 uint32_t(E[q] >> 32)};
            so.idx[pos] = uint32_t(i);
            if (d.init)
                so.init[pos] = in0[q];
        }
    }
}


}  // namespace
