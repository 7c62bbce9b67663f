// A secondary index over the replay table (ramcrc_replay_table_index_build_device,
// ramcrc_index_lookup_device, DESIGN.md 5.21): k_ix_size, k_ix_scan, k_ix_emit,
// k_ix_sort, k_ix_merge, k_ix_hashes (the build), k_ixl_search, k_ixl_scan,
// k_ixl_copy, k_ixl_long (the lookup).  Part of ramcrc_device.hip (one translation unit);
// included only from there, after dev_read_hashes.inc, whose slot decoding and
// record hash it uses; not a standalone header.
//
// The build walks the slots, not the buckets: a lane has a slot.  No workgroup
// waits for another, and the number of launches follows entry_capacity, which
// the host knows, never the number of entries, which it does not:
//   k_ix_size    one slot per lane in tiles of kPartThreads: the selection
//                (index_rules.h), per tile the entries, their key bytes and the
//                objects seen, by one atomic per wave and sum into a line the
//                call zeroed;
//   k_ix_scan    one workgroup: the tile sums become exclusive offsets; the
//                summary; the head words (entries, overflow) for what follows;
//   k_ix_emit    the selection again, a tile-local scan behind the tile's
//                offsets, the unsorted entries and the copies of their keys;
//   k_ix_sort    tiles of kIxTile entries sorted in LDS (a bitonic network
//                over whole 32-byte entries, padding above every entry);
//   k_ix_merge   one pass: runs of W entries merged in pairs.  A workgroup owns
//                kIxTile outputs: two lanes find its two ends on the pair's
//                merge path in global memory, the workgroup stages the at most
//                kIxTile inputs between them in LDS, and every lane finds its
//                own kIxPer outputs on the merge path in LDS.  Ties take the
//                first run's entry.  The passes ping-pong between d_entries
//                and context scratch and end in d_entries;
//   k_ix_hashes  d_hashes[i] = d_entries[i].pk_hash.
// The comparator decides by prefix alone when prefixes differ and reads key
// bytes from d_index_keys only for equal prefixes where both keys are longer
// than 8, never at or past key_len.
//
// The lookup is the multi-read's shape:
//   k_ixl_search one query per lane: the two binary searches, per query {lo,
//                count} into scratch, per tile the sums;
//   k_ixl_scan   one workgroup: offsets, the cut at out_capacity, the summary;
//   k_ixl_copy   per tile the offsets of its queries, the results, and the
//                short runs of hashes, 8 lanes a run (whole 64-bit words at
//                8-byte aligned places: the append's granule copy has nothing
//                to add here);
//   k_ixl_long   the runs of kIxLongRun hashes and more: the scan listed the
//                tiles that have one, and every workgroup of the grid takes
//                its stride of every such run, so that a few wide ranges are
//                copied by the whole device and not by their tiles' workgroups.

namespace {

constexpr uint32_t kIxTile = 1024;                      // entries of a sort tile: 32 KiB of LDS
constexpr uint32_t kIxPer = kIxTile / kPartThreads;     // outputs per lane of a merge
constexpr uint32_t kIxTileWords = 3;    // a tile's sums: entries, key bytes (then their offsets), objects seen
constexpr uint32_t kIxTileStride = 8;   // scratch words per tile: one 64-byte line
constexpr uint32_t kIxLongRun = kPartThreads;           // hashes from which the workgroup copies a run
enum : uint32_t {
    kIxHeadN = 0,          // entries written
    kIxHeadSkip = 1,       // nonzero: overflow, nothing is written
};
enum : uint32_t {
    kIxlHeadServed = 0,    // the leading queries that are served
    kIxlHeadLong = 1,      // tiles with a long run, listed in word kIxlTileList of the leading tile lines
};
constexpr uint32_t kIxlTileWords = 4;   // a tile's sums: hashes (then the offset), bad, maxed out, long runs
constexpr uint32_t kIxlTileList = 4;    // tile line k, word 4: the k-th tile with a long run
constexpr uint64_t kIxlMore = 1ull << 32, kIxlBad = 1ull << 33;   // a query's second scratch word: num | flags
static_assert(sizeof(ramcrc_index_entry) == 32 && sizeof(ramcrc_index_build_summary) == 56, "index ABI");
static_assert(sizeof(ramcrc_index_query) == 40 && sizeof(ramcrc_index_result) == 48 &&
              sizeof(ramcrc_index_lookup_summary) == 48, "index lookup ABI");
static_assert(kIxTile % kPartThreads == 0 && (kIxTile & (kIxTile - 1)) == 0, "a bitonic tile");

struct IxDesc {
    uint64_t table_id;
    uint32_t index_id;
    ramcrc_index_entry* entries;
    uint64_t ecap;
    uint64_t* hashes;
    uint64_t keys;                  // d_index_keys
    uint64_t kcap;
    ramcrc_index_build_summary* summary;
    uint64_t* tile;                 // scratch [kIxTileStride * tiles of slots]
    unsigned long long* head;       // scratch line
};

// Key bytes from byte 8 on, for the comparator.
struct IxTail {
    uint64_t at;
    __device__ __forceinline__ uint32_t operator[](uint32_t i) const
    {
        typedef __attribute__((address_space(1))) const uint8_t gr8;
        return *reinterpret_cast<gr8*>(at + i);
    }
};

__device__ __forceinline__ ramcrc_ix::KeyRef<IxTail> ix_ref(const ramcrc_index_entry& e, uint64_t keys)
{
    return ramcrc_ix::KeyRef<IxTail>{e.prefix, e.key_len, IxTail{keys + e.key_off + ramcrc_ix::kPrefixBytes}};
}

// The build's order; a tile's padding is above every entry.
__device__ __forceinline__ bool ix_less(const ramcrc_index_entry& x, const ramcrc_index_entry& y, uint64_t keys)
{
    if (x.key_len == ramcrc_ix::kPadLen)
        return false;
    if (y.key_len == ramcrc_ix::kPadLen)
        return true;
    return ramcrc_ix::entry_less(ix_ref(x, keys), x.pk_hash, ix_ref(y, keys), y.pk_hash);
}

struct IxAny {
    __device__ __forceinline__ bool operator()(uint64_t) const { return true; }
};

// What slot s gives the index.
struct IxSel {
    bool seen;        // an object winner of the table id
    uint64_t hash;    // its record hash
    uint64_t src;     // the key's address
    uint32_t len;     // 0: no entry
};

__device__ __forceinline__ IxSel ix_select(const RtabDesc& a, const IxDesc& r, uint64_t s)
{
    IxSel o{false, 0ull, 0ull, 0u};
    const uint64_t c = *rtab_word(a, s, 2);
    if (c == 0)
        return o;
    const uint64_t pick = *rtab_word(a, s, 1);
    if (pick == 0 || !rtab_pick_object(pick))   // (between adds every claimed slot has a pick)
        return o;
    uint64_t h;
    if (!rh_claimant(a, r.table_id, c, IxAny{}, &h))
        return o;
    const RtabWin w = rtab_decode_pick(a, pick);
    const ramcrc_ix::KeyAt k = ramcrc_ix::key_at(w.row.z, w.rd, r.index_id);
    o.seen = true;
    o.hash = h;
    o.src = w.rd.pay + k.off;
    o.len = k.len;
    return o;
}

// ---------------------------------------------------------------- k_ix_size
__global__ __launch_bounds__(kPartThreads) void k_ix_size(RtabDesc a, IxDesc r)
{
    if (rtab_refused(a))
        return;
    const uint64_t ntiles = (a.nslots + kPartThreads - 1) / kPartThreads;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t s = tile * kPartThreads + threadIdx.x;
        IxSel o{false, 0ull, 0ull, 0u};
        if (s < a.nslots)
            o = ix_select(a, r, s);
        uint64_t sums[kIxTileWords] = {o.len ? 1ull : 0ull, o.len, o.seen ? 1ull : 0ull};
#pragma unroll
        for (uint32_t k = 0; k < kIxTileWords; k++) {
            unsigned long long v = sums[k];
#pragma unroll
            for (int d = 1; d < kWaveSize; d <<= 1)
                v += __shfl_xor(v, d);
            if ((threadIdx.x & (kWaveSize - 1)) == 0 && v)
                atomicAdd(reinterpret_cast<unsigned long long*>(r.tile + kIxTileStride * tile + k), v);
        }
    }
}

// ---------------------------------------------------------------- k_ix_scan
__global__ __launch_bounds__(kPartThreads) void k_ix_scan(RtabDesc a, IxDesc r)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    const uint32_t t = threadIdx.x;
    if (rtab_refused(a)) {
        if (t == 0) {
            ramcrc_index_build_summary sm{};
            sm.spoiled = 1;
            *r.summary = sm;
            r.head[kIxHeadN] = 0;
            r.head[kIxHeadSkip] = 1;
        }
        return;
    }
    const uint64_t ntiles = (a.nslots + kPartThreads - 1) / kPartThreads;
    uint64_t ce = 0, ck = 0, seen = 0;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += kPartThreads) {
        const uint64_t tl = t0 + t;
        uint64_t* const ts = r.tile + kIxTileStride * tl;
        const uint64_t ve = tl < ntiles ? ts[0] : 0ull, vk = tl < ntiles ? ts[1] : 0ull;
        seen += tl < ntiles ? ts[2] : 0ull;
        uint64_t te, tk;
        const uint64_t be = ce + part_block_excl(ve, wsum, &te);
        const uint64_t bk = ck + part_block_excl(vk, wsum, &tk);
        if (tl < ntiles) {
            ts[0] = be;
            ts[1] = bk;
        }
        ce += te;
        ck += tk;
    }
    seen = rtab_block_sum(seen, wsum);
    if (t == 0) {
        const bool over = ramcrc_ix::overflow(ce, ck, r.ecap, r.kcap);
        ramcrc_index_build_summary sm{};
        sm.n_entries = over ? 0 : ce;
        sm.key_bytes = over ? 0 : ck;
        sm.entries_needed = ce;
        sm.key_bytes_needed = ck;
        sm.objects_seen = seen;
        sm.overflow = over;
        *r.summary = sm;
        r.head[kIxHeadN] = sm.n_entries;
        r.head[kIxHeadSkip] = over;
    }
}

// ---------------------------------------------------------------- k_ix_emit
__global__ __launch_bounds__(kPartThreads) void k_ix_emit(RtabDesc a, IxDesc r)
{
    typedef __attribute__((address_space(1))) uint8_t gw8;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    if (rtab_refused(a) || r.head[kIxHeadSkip])
        return;
    const uint64_t ntiles = (a.nslots + kPartThreads - 1) / kPartThreads;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t s = tile * kPartThreads + threadIdx.x;
        IxSel o{false, 0ull, 0ull, 0u};
        if (s < a.nslots)
            o = ix_select(a, r, s);
        uint64_t tot;
        const uint64_t idx = r.tile[kIxTileStride * tile] + part_block_excl(o.len ? 1ull : 0ull, wsum, &tot);
        const uint64_t off = r.tile[kIxTileStride * tile + 1] + part_block_excl(o.len, wsum, &tot);
        // (the scan sent only what fits; checked again as the last thing
        // between a stale word and a stray store)
        if (o.len == 0 || idx >= r.ecap || off + o.len > r.kcap)
            continue;
        uint64_t prefix = 0;
        for (uint32_t i = 0; i < o.len; i += 8) {
            const uint32_t n = o.len - i < 8 ? o.len - i : 8u;
            const uint64_t v = part_bytes(o.src + i, n);   // little-endian, zero above byte n
            if (i == 0)
                prefix = __builtin_bswap64(v);
            for (uint32_t b = 0; b < n; b++)
                *reinterpret_cast<gw8*>(r.keys + off + i + b) = uint8_t(v >> (8 * b));
        }
        r.entries[idx] = ramcrc_ix::make_entry(prefix, o.hash, off, o.len);
    }
}

// ---------------------------------------------------------------- k_ix_sort
// Tiles of kIxTile entries, each sorted in LDS; dst is d_entries or the
// scratch buffer, whichever leaves the last merge pass writing d_entries.
__global__ __launch_bounds__(kPartThreads) void k_ix_sort(RtabDesc a, IxDesc r, ramcrc_index_entry* dst)
{
    __shared__ ramcrc_index_entry se[kIxTile];
    if (rtab_refused(a) || r.head[kIxHeadSkip])
        return;
    const uint64_t n = r.head[kIxHeadN];
    const uint64_t ntiles = (n + kIxTile - 1) / kIxTile;
    const uint32_t t = threadIdx.x;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t g0 = tile * kIxTile;
#pragma unroll
        for (uint32_t k = 0; k < kIxPer; k++) {
            const uint32_t i = t + k * kPartThreads;
            if (g0 + i < n)
                se[i] = r.entries[g0 + i];
            else
                se[i] = ramcrc_index_entry{0ull, 0ull, 0ull, ramcrc_ix::kPadLen, 0u};
        }
        for (uint32_t k = 2; k <= kIxTile; k <<= 1) {
            for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                __syncthreads();
                for (uint32_t q = t; q < kIxTile / 2; q += kPartThreads) {
                    const uint32_t i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                    const ramcrc_index_entry x = se[i], y = se[l];
                    const bool up = (i & k) == 0;
                    if (up ? ix_less(y, x, r.keys) : ix_less(x, y, r.keys)) {
                        se[i] = y;
                        se[l] = x;
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kIxPer; k++) {
            const uint32_t i = t + k * kPartThreads;
            if (g0 + i < n)
                dst[g0 + i] = se[i];
        }
        __syncthreads();   // se is free again
    }
}

// How many of the first d outputs of merging A[0, na) and B[0, nb) come from
// A, where ties take A's: the first i with B[d - 1 - i] < A[i].
__device__ __forceinline__ uint64_t ix_merge_path(const ramcrc_index_entry* A, uint64_t na,
                                                  const ramcrc_index_entry* B, uint64_t nb, uint64_t d,
                                                  uint64_t keys)
{
    uint64_t lo = d > nb ? d - nb : 0ull, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (ix_less(B[d - 1 - mid], A[mid], keys))
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// --------------------------------------------------------------- k_ix_merge
// One pass: the runs [2pW, 2pW + W) and [2pW + W, 2pW + 2W), cut at n, merged
// from src into dst.  A last run without a partner is copied.
__global__ __launch_bounds__(kPartThreads) void k_ix_merge(RtabDesc a, IxDesc r, uint64_t W,
                                                           const ramcrc_index_entry* src,
                                                           ramcrc_index_entry* dst)
{
    __shared__ ramcrc_index_entry se[kIxTile];
    __shared__ uint64_t cut[2];
    if (rtab_refused(a) || r.head[kIxHeadSkip])
        return;
    const uint64_t n = r.head[kIxHeadN];
    const uint64_t ntiles = (n + kIxTile - 1) / kIxTile;
    const uint32_t t = threadIdx.x;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t out0 = tile * kIxTile;
        const uint64_t base = out0 / (2 * W) * (2 * W);
        const uint64_t na = n - base < W ? n - base : W;
        const uint64_t nb = n - base - na < W ? n - base - na : W;
        const ramcrc_index_entry* const A = src + base;
        const ramcrc_index_entry* const B = A + na;
        const uint64_t d0 = out0 - base;
        const uint64_t d1 = d0 + kIxTile < na + nb ? d0 + kIxTile : na + nb;
        if (t < 2)
            cut[t] = ix_merge_path(A, na, B, nb, t ? d1 : d0, r.keys);
        __syncthreads();
        const uint64_t a0 = cut[0], b0 = d0 - a0;
        const uint32_t la = uint32_t(cut[1] - a0), lb = uint32_t(d1 - d0) - la;   // la + lb <= kIxTile
        for (uint32_t i = t; i < la + lb; i += kPartThreads)
            se[i] = i < la ? A[a0 + i] : B[b0 + (i - la)];
        __syncthreads();
        const uint32_t d = t * kIxPer < la + lb ? t * kIxPer : la + lb;
        uint32_t ai = uint32_t(ix_merge_path(se, la, se + la, lb, d, r.keys)), bi = d - ai;
        for (uint32_t k = 0; k < kIxPer && d + k < la + lb; k++) {
            const bool from_a = bi >= lb || (ai < la && !ix_less(se[la + bi], se[ai], r.keys));
            dst[out0 + d + k] = from_a ? se[ai] : se[la + bi];
            ai += from_a;
            bi += !from_a;
        }
        __syncthreads();   // se and cut are free again
    }
}

// -------------------------------------------------------------- k_ix_hashes
__global__ __launch_bounds__(kPartThreads) void k_ix_hashes(RtabDesc a, IxDesc r)
{
    if (rtab_refused(a) || r.head[kIxHeadSkip])
        return;
    const uint64_t n = r.head[kIxHeadN];
    const uint64_t nthr = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += nthr)
        r.hashes[i] = r.entries[i].pk_hash;
}

// ================================================================ the lookup
struct IxlDesc {
    const ramcrc_index_entry* entries;
    const uint64_t* hashes;
    uint64_t keys;                  // d_index_keys
    const ramcrc_index_build_summary* build;
    uint64_t qkeys, qkeys_bytes;
    const uint64_t* queries;        // five words each
    uint64_t nq;
    uint64_t* out;
    uint64_t ocap;
    ramcrc_index_result* results;
    ramcrc_index_lookup_summary* summary;
    uint64_t* rec;                  // scratch [2 * nq]: lo, num | flags
    uint64_t* tile;                 // scratch [kIxTileStride * tiles]: see kIxlTileWords, kIxlTileList
    unsigned long long* head;       // scratch line
};

// Is the index unusable: its build overflowed or met a spoiled table?
__device__ __forceinline__ bool ixl_dead(const IxlDesc& r)
{
    return (r.build->overflow | r.build->spoiled) != 0;
}

__device__ __forceinline__ ramcrc_index_query ixl_query(const IxlDesc& r, uint64_t i)
{
    const uint64_t* const w = r.queries + 5 * i;
    ramcrc_index_query q;
    q.first_off = w[0];
    q.last_off = w[1];
    q.first_allowed_hash = w[2];
    q.first_len = uint32_t(w[3]);
    q.last_len = uint32_t(w[3] >> 32);
    q.max_hashes = uint32_t(w[4]);
    q.reserved = uint32_t(w[4] >> 32);
    return q;
}

// ------------------------------------------------------------- k_ixl_search
__global__ __launch_bounds__(kPartThreads) void k_ixl_search(IxlDesc r)
{
    namespace ix = ramcrc_ix;
    if (ixl_dead(r))
        return;
    const uint64_t n = r.build->n_entries;
    const uint64_t ntiles = (r.nq + kPartThreads - 1) / kPartThreads;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i = tile * kPartThreads + threadIdx.x;
        uint64_t num = 0, bad = 0, more = 0;
        if (i < r.nq) {
            const ramcrc_index_query q = ixl_query(r, i);
            uint64_t lo = 0;
            if (ix::bad_query(q, r.qkeys_bytes)) {
                bad = 1;
            } else {
                const IxTail f0{r.qkeys + q.first_off}, l0{r.qkeys + q.last_off};
                const ix::KeyRef<IxTail> first{ix::prefix_of(f0, q.first_len), q.first_len,
                                               IxTail{f0.at + ix::kPrefixBytes}};
                const ix::KeyRef<IxTail> last{ix::prefix_of(l0, q.last_len), q.last_len,
                                              IxTail{l0.at + ix::kPrefixBytes}};
                lo = ix::first_false(n, [&](uint64_t m) {
                    const ramcrc_index_entry e = r.entries[m];
                    return ix::entry_less(ix_ref(e, r.keys), e.pk_hash, first, q.first_allowed_hash);
                });
                uint64_t hi = n;
                if (q.last_len)
                    hi = ix::first_false(n, [&](uint64_t m) {
                        return ix::key_compare(ix_ref(r.entries[m], r.keys), last) <= 0;
                    });
                const ix::Answer an = ix::answer(lo, hi, q.max_hashes);
                num = an.num;
                more = an.more;
            }
            r.rec[2 * i] = lo;
            r.rec[2 * i + 1] = num | (more ? kIxlMore : 0ull) | (bad ? kIxlBad : 0ull);
        }
        uint64_t sums[kIxlTileWords] = {num, bad, more, num >= kIxLongRun ? 1ull : 0ull};
#pragma unroll
        for (uint32_t k = 0; k < kIxlTileWords; k++) {
            unsigned long long v = sums[k];
#pragma unroll
            for (int d = 1; d < kWaveSize; d <<= 1)
                v += __shfl_xor(v, d);
            if ((threadIdx.x & (kWaveSize - 1)) == 0 && v)
                atomicAdd(reinterpret_cast<unsigned long long*>(r.tile + kIxTileStride * tile + k), v);
        }
    }
}

// --------------------------------------------------------------- k_ixl_scan
// One workgroup.  The ends of the queries' hashes grow with the query, so the
// served queries are a prefix: whole tiles, then a prefix of one tile.
__global__ __launch_bounds__(kPartThreads) void k_ixl_scan(IxlDesc r)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ unsigned long long cut_s;
    const uint32_t t = threadIdx.x;
    if (ixl_dead(r)) {
        if (t == 0) {
            ramcrc_index_lookup_summary sm{};
            sm.overflow_index = 1;
            *r.summary = sm;
            r.head[kIxlHeadServed] = 0;
        }
        return;
    }
    const uint64_t ntiles = (r.nq + kPartThreads - 1) / kPartThreads;
    if (t == 0)
        cut_s = ntiles;
    __syncthreads();
    uint64_t carry = 0, cut = ntiles, bad = 0, maxed = 0;
    for (uint64_t t0 = 0; t0 < ntiles; t0 += kPartThreads) {
        const uint64_t tl = t0 + t;
        uint64_t* const ts = r.tile + kIxTileStride * tl;
        const uint64_t v = tl < ntiles ? ts[0] : 0ull;
        uint64_t tot;
        const uint64_t base = carry + part_block_excl(v, wsum, &tot);
        if (tl < ntiles) {
            ts[0] = base;
            if (base + v <= r.ocap) {
                bad += ts[1];
                maxed += ts[2];
            } else if (tl < cut) {
                cut = tl;
            }
            // (the list's word is no tile's sum: nobody reads it before k_ixl_long)
            if (ts[3])
                r.tile[kIxTileStride * atomicAdd(&r.head[kIxlHeadLong], 1ull) + kIxlTileList] = tl;
        }
        carry += tot;
    }
    if (cut < ntiles)
        atomicMin(&cut_s, static_cast<unsigned long long>(cut));
    __syncthreads();   // the cut, and every tile's offset
    cut = cut_s;
    // (a tile behind the cut has counted nothing: the ends grow with the tile)
    uint64_t served = r.nq, hashes = carry;
    if (cut < ntiles) {
        // the tile the output ends in: its queries one by one
        const uint64_t i = cut * kPartThreads + t;
        const uint64_t w = i < r.nq ? r.rec[2 * i + 1] : 0ull;
        const uint32_t num = uint32_t(w);
        uint64_t tot;
        const uint64_t base = r.tile[kIxTileStride * cut];
        const uint64_t off = base + part_block_excl(num, wsum, &tot);
        const bool in = i < r.nq && ramcrc_ix::served(off, num, r.ocap);
        bad += in && (w & kIxlBad);
        maxed += in && (w & kIxlMore);
        served = cut * kPartThreads + rtab_block_sum(in ? 1ull : 0ull, wsum);
        hashes = base + rtab_block_sum(in ? uint64_t(num) : 0ull, wsum);
    }
    bad = rtab_block_sum(bad, wsum);
    maxed = rtab_block_sum(maxed, wsum);
    if (t == 0) {
        ramcrc_index_lookup_summary sm{};
        sm.served = served;
        sm.hashes = hashes;
        sm.bad = bad;
        sm.maxed_out = maxed;
        sm.n_entries = r.build->n_entries;
        *r.summary = sm;
        r.head[kIxlHeadServed] = served;
    }
}

// --------------------------------------------------------------- k_ixl_copy
__global__ __launch_bounds__(kPartThreads) void k_ixl_copy(IxlDesc r)
{
    namespace ix = ramcrc_ix;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ uint64_t ssrc[kPartThreads], sdst[kPartThreads];
    __shared__ uint32_t snum[kPartThreads];
    const uint64_t served = r.head[kIxlHeadServed];
    const uint64_t ntiles = (r.nq + kPartThreads - 1) / kPartThreads;
    const uint32_t t = threadIdx.x;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i = tile * kPartThreads + t;
        const bool in = i < served;   // (served <= nq; a dead index serves none and has no sums)
        const uint64_t lo = in ? r.rec[2 * i] : 0ull, w = in ? r.rec[2 * i + 1] : 0ull;
        const uint32_t num = uint32_t(w);
        uint64_t tot;
        const uint64_t off = (in ? r.tile[kIxTileStride * tile] : 0ull) + part_block_excl(num, wsum, &tot);
        if (i < r.nq) {
            ramcrc_index_result res = ix::no_result(RAMCRC_INDEX_NOT_SERVED);
            if (in && (w & kIxlBad)) {
                res = ix::no_result(RAMCRC_INDEX_BAD_QUERY);
            } else if (in) {
                res = ramcrc_index_result{off, 0ull, 0ull, 0ull, num, 0u, RAMCRC_INDEX_OK, 0u};
                if (w & kIxlMore) {
                    const ramcrc_index_entry e = r.entries[lo + num];
                    res.next_entry = lo + num;
                    res.next_key_hash = e.pk_hash;
                    res.next_key_off = e.key_off;
                    res.next_key_len = e.key_len;
                }
            }
            r.results[i] = res;
        }
        ssrc[t] = lo;
        sdst[t] = off;
        // (checked again as the last thing between a stale word and a stray store)
        snum[t] = in && ix::served(off, num, r.ocap) ? num : 0u;
        __syncthreads();
        const uint32_t g = t >> 3, sub = t & 7;
        for (uint32_t j = g; j < kPartThreads; j += kPartThreads / 8) {
            const uint32_t nn = snum[j];
            if (nn && nn < kIxLongRun)
                for (uint32_t k = sub; k < nn; k += 8)
                    r.out[sdst[j] + k] = r.hashes[ssrc[j] + k];
        }
        __syncthreads();   // the lists are free again
    }
}

// --------------------------------------------------------------- k_ixl_long
__global__ __launch_bounds__(kPartThreads) void k_ixl_long(IxlDesc r)
{
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ uint64_t ssrc[kPartThreads], sdst[kPartThreads];
    __shared__ uint32_t snum[kPartThreads];
    const uint64_t served = r.head[kIxlHeadServed], nlong = r.head[kIxlHeadLong];
    const uint32_t t = threadIdx.x;
    for (uint64_t li = 0; li < nlong; li++) {
        const uint64_t tile = r.tile[kIxTileStride * li + kIxlTileList];
        const uint64_t i = tile * kPartThreads + t;
        const bool in = i < served;
        const uint64_t lo = in ? r.rec[2 * i] : 0ull;
        const uint32_t num = in ? uint32_t(r.rec[2 * i + 1]) : 0u;
        uint64_t tot;
        const uint64_t off = r.tile[kIxTileStride * tile] + part_block_excl(num, wsum, &tot);
        ssrc[t] = lo;
        sdst[t] = off;
        snum[t] = num >= kIxLongRun && ramcrc_ix::served(off, num, r.ocap) ? num : 0u;
        __syncthreads();
        for (uint32_t j = 0; j < kPartThreads; j++) {
            const uint32_t nn = snum[j];
            for (uint64_t k = uint64_t(blockIdx.x) * kPartThreads + t; k < nn; k += uint64_t(gridDim.x) * kPartThreads)
                r.out[sdst[j] + k] = r.hashes[ssrc[j] + k];
        }
        __syncthreads();   // the lists are free again
    }
}

}  // namespace
