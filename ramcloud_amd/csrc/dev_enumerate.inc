// One reply of a table enumeration (ramcrc_replay_table_enumerate_device,
// DESIGN.md 5.20): k_en_size, k_en_scan, k_en_gather.  Part of
// ramcrc_device.hip (one translation unit); included only from there, after
// dev_read_hashes.inc, whose slot decoding and record-hash test it uses; not a
// standalone header.
//
// The first call whose walk starts from the table and not from a request: a
// lane has a bucket b, not a key.  The bucket's keys are the claimed slots
// between slot b and the first unclaimed one whose record hash has home b
// (slots are never un-claimed); the walk wraps and is bounded by the slot
// count, as rh_find's is.  The launch shape is the multi-read's; no workgroup
// waits for another:
//   k_en_size    one bucket per lane in tiles of kPartThreads: the chain, the
//                selection (enumerate_rules.h), per bucket the bytes of its
//                entries, its objects and tombstones, value and key bytes;
//                nothing is kept per bucket: per tile the sums, by one atomic
//                per wave and sum into a line the call zeroed;
//   k_en_scan    one workgroup: the tile sums become exclusive offsets; the
//                tiles that end within lim count whole; the lanes walk the
//                buckets of the first tile that does not again for the first
//                bucket that is not kept whole; if that is bucket_index
//                itself, its lane takes the entries in order for the cut
//                inside it; then the summary and the head words for the gather;
//   k_en_gather  per tile the lanes walk their buckets a second time: the
//                sizes, for the offsets by a tile-local scan, and in the same
//                walk the bucket's first kEnPer entries in {hash, batch,
//                record} order, kept sorted in registers.  Then passes: in
//                each, every lane that still has entries posts up to kEnPer
//                of them to a list in LDS, and the tile copies what was
//                posted as k_rtab_read_gather does (app_copy and its size
//                classes; the 4 length bytes, which may begin at any byte, as
//                byte stores).  A bucket with two or three objects is ordinary
//                here (about one in eleven at load 0.5) and costs nothing
//                more; one with more than kEnPer costs its tile a pass, with
//                one more walk from the last entry sent, per kEnPer entries.
// Scratch grows with tiles, not with buckets or objects: kEnTileStride words a
// tile and the head line.  The price is the gather's second walk.

namespace {

constexpr uint32_t kEnTileWords = 5;    // a tile's sums: bytes (then the offset), objects, tombstones,
                                        // value bytes, key bytes
constexpr uint32_t kEnTileStride = 8;   // scratch words per tile: one 64-byte line, which no other
                                        // tile's atomics share
constexpr uint32_t kEnScanPer = 2;      // tiles per lane and step of the scan
// The head line, written by the scan for the gather.
enum : uint32_t {
    kEnHeadWhole = 0,     // buckets kept whole, counted from bucket_index
    kEnHeadPartial = 1,   // nonzero: bucket_index itself is sent in part ...
    kEnHeadCutHash = 2,   // ... its hashes below this
    kEnHeadBytes = 3,     // payload_bytes: no store at or past it
};
static_assert(sizeof(ramcrc_enum_frame) == 40 && sizeof(ramcrc_enumerate_summary) == 88, "enumerate ABI");
static_assert(kAppCopyThreads == kPartThreads, "a tile's lanes copy what its lanes posted");

struct EnDesc {
    uint64_t table_id;
    uint64_t nb;                    // buckets of the call: from bucket_index to the bucket limit
    uint64_t payload;
    uint64_t lim;                   // min(max_bytes, payload_capacity)
    ramcrc_enumerate_summary* summary;
    uint64_t* tile;                 // scratch [kEnTileStride * tiles]
    unsigned long long* head;       // scratch line
    uint32_t flags;
    ramcrc_en::Select sel;
};

// A walk's test of a record hash: home b, selected, and before the cut.
struct EnWanted {
    const ramcrc_en::Select* sel;
    uint64_t b, mask, cut_hash;
    bool cut;
    __device__ __forceinline__ bool operator()(uint64_t h) const
    {
        return (h & mask) == b && ramcrc_en::selected(*sel, b, h) &&
               ramcrc_en::before_cut(*sel, b, h, cut, cut_hash);
    }
};

// What bucket b holds of the selection.
__device__ __forceinline__ ramcrc_en::Found en_size(const RtabDesc& a, const EnDesc& r, uint64_t b)
{
    namespace en = ramcrc_en;
    en::Found f = en::nothing();
    const uint64_t mask = a.nslots - 1;
    const EnWanted wanted{&r.sel, b, mask, 0, false};
    uint64_t s = b & mask;
    // bounded by the slot count, as the insert's probe is
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint64_t c = *rtab_word(a, s, 2);
        if (c == 0)
            break;
        uint64_t h;
        if (!rh_claimant(a, r.table_id, c, wanted, &h))
            continue;
        const uint64_t pick = *rtab_word(a, s, 1);
        if (pick == 0)   // (between adds every claimed slot has one)
            continue;
        if (!rtab_pick_object(pick)) {
            f.tombstones++;
            continue;
        }
        const RtabWin w = rtab_decode_pick(a, pick);
        en::add_object(&f, r.flags, w.row.z, ramcrc_look::object_value(w.row.z, w.rd));
    }
    return f;
}

// An entry of a bucket.
struct EnEntry {
    uint64_t hash, order;
    uint64_t src;             // its payload
    uint32_t len;             // the payload's length
    ramcrc_look::Value v;     // (kValue) the value's place
};

// The object of bucket b with the smallest {hash, order} at or above {fh, fo};
// false: there is none.  kValue: with the value's place, which costs a read of
// the payload.
template <bool kValue>
__device__ __forceinline__ bool en_next(const RtabDesc& a, const EnDesc& r, uint64_t b, bool cut, uint64_t cut_hash,
                                        uint64_t fh, uint64_t fo, EnEntry* e)
{
    namespace en = ramcrc_en;
    const uint64_t mask = a.nslots - 1;
    const EnWanted wanted{&r.sel, b, mask, cut_hash, cut};
    uint64_t s = b & mask, bh = ~0ull, bo = ~0ull, best_pick = 0;
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint64_t c = *rtab_word(a, s, 2);
        if (c == 0)
            break;
        const uint64_t pick = *rtab_word(a, s, 1);
        if (pick == 0 || !rtab_pick_object(pick))
            continue;
        uint64_t h;
        if (!rh_claimant(a, r.table_id, c, wanted, &h))
            continue;
        const uint64_t o = en::order_of(rtab_pick_batch(pick), rtab_pick_record(pick));
        // (an order is below 2^48, so {~0, ~0} is above every entry)
        if (!en::at_or_above(h, o, fh, fo) || !en::below(h, o, bh, bo))
            continue;
        bh = h;
        bo = o;
        best_pick = pick;
    }
    if (best_pick == 0)
        return false;
    const RtabWin w = rtab_decode_pick(a, best_pick);
    e->hash = bh;
    e->order = bo;
    e->src = w.rd.pay;
    e->len = w.row.z;
    e->v = ramcrc_look::Value{w.row.z, 0u};
    if (kValue || (r.flags & RAMCRC_ENUM_KEYS_ONLY))
        e->v = ramcrc_look::object_value(w.row.z, w.rd);
    return true;
}

// The gather's walk: a bucket's first kEnPer entries at or above {fh, fo}, in
// order, each with its source and its `length`; *bytes and *objects: of all
// its entries at or above {fh, fo}.  The entries stay in registers (every index
// below is a constant after unrolling); a bucket with more costs another walk.
constexpr uint32_t kEnPer = 3;

struct EnFew {
    uint64_t hash[kEnPer], order[kEnPer], src[kEnPer];
    uint32_t length[kEnPer];
    uint32_t n;
};

__device__ __forceinline__ void en_few(const RtabDesc& a, const EnDesc& r, uint64_t b, bool cut, uint64_t cut_hash,
                                       uint64_t fh, uint64_t fo, EnFew* few, uint64_t* bytes, uint64_t* objects)
{
    namespace en = ramcrc_en;
    const uint64_t mask = a.nslots - 1;
    const EnWanted wanted{&r.sel, b, mask, cut_hash, cut};
#pragma unroll
    for (uint32_t k = 0; k < kEnPer; k++) {
        few->hash[k] = few->order[k] = ~0ull;   // (an order is below 2^48: above every entry)
        few->src[k] = 0;
        few->length[k] = 0;
    }
    uint64_t nb = 0, no = 0;
    uint64_t s = b & mask;
    for (uint64_t step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const uint64_t c = *rtab_word(a, s, 2);
        if (c == 0)
            break;
        const uint64_t pick = *rtab_word(a, s, 1);
        if (pick == 0 || !rtab_pick_object(pick))
            continue;
        uint64_t h;
        if (!rh_claimant(a, r.table_id, c, wanted, &h))
            continue;
        uint64_t o = en::order_of(rtab_pick_batch(pick), rtab_pick_record(pick));
        if (!en::at_or_above(h, o, fh, fo))
            continue;
        const RtabWin w = rtab_decode_pick(a, pick);
        ramcrc_look::Value v{w.row.z, 0u};
        if (r.flags & RAMCRC_ENUM_KEYS_ONLY)
            v = ramcrc_look::object_value(w.row.z, w.rd);
        uint32_t length = en::entry_length(r.flags, w.row.z, v);
        uint64_t src = w.rd.pay;
        nb += en::entry_size(length);
        no++;
        // insertion: the entry in hand sinks to its place, the largest drops out
#pragma unroll
        for (uint32_t k = 0; k < kEnPer; k++) {
            if (en::below(h, o, few->hash[k], few->order[k])) {
                const uint64_t th = few->hash[k], to = few->order[k], ts = few->src[k];
                const uint32_t tl = few->length[k];
                few->hash[k] = h;
                few->order[k] = o;
                few->src[k] = src;
                few->length[k] = length;
                h = th;
                o = to;
                src = ts;
                length = tl;
            }
        }
    }
    few->n = uint32_t(no < kEnPer ? no : kEnPer);
    *bytes = nb;
    *objects = no;
}

// ---------------------------------------------------------------- k_en_size
__global__ __launch_bounds__(kPartThreads) void k_en_size(RtabDesc a, EnDesc r)
{
    namespace en = ramcrc_en;
    if (rtab_refused(a))
        return;
    const uint64_t ntiles = (r.nb + kPartThreads - 1) / kPartThreads;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i = tile * kPartThreads + threadIdx.x;
        en::Found f = en::nothing();
        if (i < r.nb)
            f = en_size(a, r, r.sel.bucket_index + i);
        // the tile's sums, which the call zeroed: one atomic per wave and sum,
        // so that no wave waits for another, as in the multi-read
        uint64_t sums[kEnTileWords] = {f.bytes, f.objects, f.tombstones, f.value_bytes, f.key_bytes};
#pragma unroll
        for (uint32_t k = 0; k < kEnTileWords; k++) {
            unsigned long long v = sums[k];
#pragma unroll
            for (int d = 1; d < kWaveSize; d <<= 1)
                v += __shfl_xor(v, d);
            if ((threadIdx.x & (kWaveSize - 1)) == 0 && v)
                atomicAdd(reinterpret_cast<unsigned long long*>(r.tile + kEnTileStride * tile + k), v);
        }
    }
}

// ---------------------------------------------------------------- k_en_scan
// One workgroup.  The ends of the buckets' entries grow with the bucket, so
// the buckets kept whole are a prefix: whole tiles, then a prefix of one tile.
__global__ __launch_bounds__(kPartThreads) void k_en_scan(RtabDesc a, EnDesc r)
{
    namespace en = ramcrc_en;
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ unsigned long long cut_s;
    const uint32_t t = threadIdx.x;
    if (rtab_refused(a)) {
        if (t == 0) {
            ramcrc_enumerate_summary sm{};
            sm.spoiled = 1;
            *r.summary = sm;
        }
        return;
    }
    const uint64_t ntiles = (r.nb + kPartThreads - 1) / kPartThreads;
    if (t == 0)
        cut_s = ntiles;
    __syncthreads();
    uint64_t carry = 0, cut = ntiles;
    uint64_t cnt[kEnTileWords - 1] = {};   // objects, tombstones, value bytes, key bytes
    for (uint64_t t0 = 0; t0 < ntiles; t0 += uint64_t(kPartThreads) * kEnScanPer) {
        // kEnScanPer neighbouring tiles a lane, their loads in flight together
        const uint64_t tl0 = t0 + uint64_t(t) * kEnScanPer;
        uint64_t v[kEnScanPer], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kEnScanPer; k++) {
            v[k] = tl0 + k < ntiles ? r.tile[kEnTileStride * (tl0 + k)] : 0ull;
            sum += v[k];
        }
        uint64_t tot;
        uint64_t base = carry + part_block_excl(sum, wsum, &tot);
#pragma unroll
        for (uint32_t k = 0; k < kEnScanPer; k++) {
            const uint64_t tl = tl0 + k;
            if (tl >= ntiles)
                break;
            uint64_t* const ts = r.tile + kEnTileStride * tl;
            ts[0] = base;
            if (base + v[k] <= r.lim) {
#pragma unroll
                for (uint32_t j = 1; j < kEnTileWords; j++)
                    cnt[j - 1] += ts[j];
            } else if (tl < cut) {
                cut = tl;
            }
            base += v[k];
        }
        carry += tot;
    }
    if (cut < ntiles)
        atomicMin(&cut_s, static_cast<unsigned long long>(cut));
    __syncthreads();   // the cut, and every tile's offset
    cut = cut_s;
    // (a tile behind the cut has counted nothing: the ends grow with the tile)
    uint64_t whole = r.nb, bytes = carry;
    if (cut < ntiles) {
        // the tile the payload ends in: its buckets once more, one by one
        const uint64_t i = cut * kPartThreads + t;
        en::Found f = en::nothing();
        if (i < r.nb)
            f = en_size(a, r, r.sel.bucket_index + i);
        uint64_t tot;
        const uint64_t base = r.tile[kEnTileStride * cut];
        const uint64_t off = base + part_block_excl(f.bytes, wsum, &tot);
        const bool in = i < r.nb && off + f.bytes <= r.lim;
        if (in) {
            cnt[0] += f.objects;
            cnt[1] += f.tombstones;
            cnt[2] += f.value_bytes;
            cnt[3] += f.key_bytes;
        }
        whole = cut * kPartThreads + rtab_block_sum(in ? 1ull : 0ull, wsum);
        bytes = base + rtab_block_sum(in ? f.bytes : 0ull, wsum);
    }
    uint64_t sums[kEnTileWords - 1];
#pragma unroll
    for (uint32_t k = 0; k < kEnTileWords - 1; k++)
        sums[k] = rtab_block_sum(cnt[k], wsum);
    if (t == 0) {
        ramcrc_enumerate_summary sm{};
        sm.num_buckets = a.nslots;
        sm.next_bucket = r.sel.bucket_index + whole;
        sm.objects = sums[0];
        sm.payload_bytes = bytes;
        sm.value_bytes = sums[2];
        sm.key_bytes = sums[3];
        sm.tombstones = sums[1];
        sm.full = whole < r.nb;
        uint64_t partial = 0, cut_hash = 0;
        if (whole == 0 && r.nb) {
            // bucket_index itself is not kept whole: its entries in order, as
            // the gather will send them, up to the cut inside it
            en::Cut c = en::cut_begin();
            uint64_t fh = 0, fo = 0;
            EnEntry e;
            while (en_next<true>(a, r, r.sel.bucket_index, false, 0, fh, fo, &e) &&
                   en::cut_entry(&c, r.lim, e.hash, r.flags, e.len, e.v)) {
                fh = e.hash;
                fo = e.order + 1;
            }
            // (c.done: the bucket's entries pass lim, or it were kept whole)
            if (c.done) {
                partial = c.sent.objects != 0;
                cut_hash = c.next_hash;
                sm.next_hash = c.next_hash;
                sm.objects = c.sent.objects;
                sm.payload_bytes = c.sent.bytes;
                sm.value_bytes = c.sent.value_bytes;
                sm.key_bytes = c.sent.key_bytes;
                sm.stuck = c.sent.objects == 0;
            }
        }
        *r.summary = sm;
        r.head[kEnHeadWhole] = whole;
        r.head[kEnHeadPartial] = partial;
        r.head[kEnHeadCutHash] = cut_hash;
        r.head[kEnHeadBytes] = sm.payload_bytes;
    }
}

// -------------------------------------------------------------- k_en_gather
__global__ __launch_bounds__(kPartThreads) void k_en_gather(RtabDesc a, EnDesc r)
{
    namespace en = ramcrc_en;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    constexpr uint32_t kPosts = kPartThreads * kEnPer;   // what a tile may post in one pass
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    __shared__ uint64_t ssrc[kPosts], sdst[kPosts];   // sdst: behind the length
    __shared__ uint32_t slen[kPosts], sbig[kPosts];
    __shared__ uint32_t npost[2], nbig[2];   // by pass parity, as in k_app_copy
    if (rtab_refused(a))
        return;
    const uint64_t whole = r.head[kEnHeadWhole], total = r.head[kEnHeadBytes];
    const bool cut = r.head[kEnHeadPartial] != 0;
    const uint64_t cut_hash = r.head[kEnHeadCutHash];
    const uint64_t nsend = whole + (cut ? 1 : 0);   // (cut: whole is 0)
    const uint64_t ntiles = (nsend + kPartThreads - 1) / kPartThreads;
    const uint32_t t = threadIdx.x;
    if (t == 0)
        npost[0] = npost[1] = nbig[0] = nbig[1] = 0;
    uint32_t par = 0;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i = tile * kPartThreads + t;
        const uint64_t b = r.sel.bucket_index + i;
        EnFew few;
        few.n = 0;
        uint64_t bytes = 0, left = 0;
        if (i < nsend)
            en_few(a, r, b, cut, cut_hash, 0, 0, &few, &bytes, &left);
        uint64_t tot;
        uint64_t off = r.tile[kEnTileStride * tile] + part_block_excl(bytes, wsum, &tot);
        uint64_t fh = 0, fo = 0;
        bool walked = true;   // `few` holds the bucket's next entries
        // passes: up to kEnPer entries of every bucket that has some left
        for (;;) {
            // (also: the previous pass's copies have read what was posted)
            if (!__syncthreads_or(left != 0))
                break;
            if (t == 0)
                npost[par ^ 1u] = nbig[par ^ 1u] = 0;   // the next pass's
            if (left) {
                if (!walked) {
                    uint64_t nb, no;
                    en_few(a, r, b, cut, cut_hash, fh, fo, &few, &nb, &no);
                }
                if (few.n == 0)
                    left = 0;
#pragma unroll
                for (uint32_t k = 0; k < kEnPer; k++) {
                    if (k < few.n && left) {
                        const uint32_t length = few.length[k];
                        // (the scan sent only what fits; checked again as the last
                        // thing between a stale word and a stray store)
                        if (off + en::entry_size(length) <= total) {
                            const uint32_t at = atomicAdd(&npost[par], 1u);
                            ssrc[at] = few.src[k];
                            sdst[at] = r.payload + off + en::kLengthBytes;
                            slen[at] = length;
                            if (length >= kAppBigMin)
                                sbig[atomicAdd(&nbig[par], 1u)] = at;
                            off += en::entry_size(length);
                            fh = few.hash[k];
                            fo = few.order[k] + 1;
                            left--;
                        } else {
                            left = 0;
                        }
                    }
                }
            }
            walked = false;
            __syncthreads();
            const uint32_t np = npost[par], g = t >> 3, sub = t & 7;
            for (uint32_t j = g; j < np; j += kPartThreads / 8) {
                const uint64_t d = sdst[j];
                const uint32_t L = slen[j];
                if (sub < en::kLengthBytes)
                    *reinterpret_cast<gw8*>(d - en::kLengthBytes + sub) = en::length_byte(L, sub);
                if (L && L <= kAppShortMax)
                    app_copy<8, 2>(ssrc[j], d, L, sub);
                else if (L > kAppShortMax && L < kAppBigMin)
                    app_copy<8, 8>(ssrc[j], d, L, sub);
            }
            const uint32_t nb = nbig[par], wv = t >> 6, ln = t & 63;
            for (uint32_t k = wv; k < nb; k += kPartThreads / kWaveSize) {
                const uint32_t j = sbig[k];
                if (slen[j] < kAppGroupMin)
                    app_copy<kWaveSize, 4>(ssrc[j], sdst[j], slen[j], ln);
            }
            for (uint32_t k = 0; k < nb; k++) {
                const uint32_t j = sbig[k];
                if (slen[j] >= kAppGroupMin)
                    app_copy<kPartThreads, 4>(ssrc[j], sdst[j], slen[j], t);
            }
            par ^= 1u;
        }
    }
}

}  // namespace
