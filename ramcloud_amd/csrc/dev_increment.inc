// A multi-increment against the replay table
// (ramcrc_replay_table_increment_device, DESIGN.md 5.18): k_rm_group,
// k_inc_size, k_wr_scan, k_inc_emit.
// Part of ramcrc_device.hip (one translation unit: the kernels share the
// g_tab tables, LDS layouts and templates without relocatable device code).
// Included only from there, after dev_remove.inc; not a standalone header.
//
// The table is only read.  Four launches, none of which waits for another
// workgroup.  The requests are the remove's and what is written is the
// write's, so two of the four are theirs, launched as they stand:
//   k_rm_group  the remove's grouping pass over the same request layout: the
//               key's hash into a scratch word, the lowest request of a key in
//               a one-word slot;
//   k_inc_size  one request per lane in tiles of kPartThreads: rtab_probe with
//               the group pass's hash, the first-of-its-key test, the outcome
//               (increment_rules.h), the old value's 8 bytes by part_bytes --
//               the aligned 16-byte word that holds the first byte and the next
//               one only when the value crosses into it, so no load leaves the
//               segment --, the sum; per request the write's four-word record
//               (the winner's version, value | image bytes << 32, the
//               tombstone's segment id, the flags) and the new bits; per tile
//               the write's five sums, stored by the one workgroup that has
//               the tile; the counts the cut does not depend on by one atomic
//               per workgroup and count on the head line;
//   k_wr_scan   the write's, over those records and sums: offsets, allocation
//               ranks, the cut, and a ramcrc_write_summary in scratch;
//   k_inc_emit  per tile the offsets again, the version, the part, the
//               reference, as k_wr_emit; then the entries.  Every output entry
//               is tiny, so the class that decides the time is the short key:
//               up to kIncLaneKeyMax key bytes a lane builds the object entry
//               and, when there is one, the tombstone entry in registers --
//               metadata, header, checksum, payload -- and stores each as
//               aligned 32-bit words between at most three head and three tail
//               bytes (inc_object_lane; rm_tombstone_lane as it stands).
//               Longer keys go to groups of 8 lanes: the object's message is
//               the 20 header bytes, the image's 3 prefix bytes, the key and
//               the 8 value bytes, split in eighths as wr_tombstone splits its
//               message; wr_tombstone serves as is.  The certificate is folded
//               and sealed as in k_wr_emit; the workgroup that seals it turns
//               the scratch summary into the caller's.

namespace {

constexpr uint32_t kIncReqWords = 7;      // scratch per request: the hash, the group slot, the record (4), the new bits
constexpr uint32_t kIncSumWords = sizeof(ramcrc_write_summary) / sizeof(uint32_t);   // k_wr_scan's summary
constexpr uint32_t kIncKinds = 6;         // doesnt_exist, object_exists, wrong_version, bad, retry_duplicate, invalid_object
constexpr uint32_t kIncLaneKeyMax = kRmLaneKeyMax;   // 36: up to here a lane builds the entries (rm_tombstone_lane's bound)
static_assert(ramcrc_write::kObjHeader + ramcrc_increment::kImagePrefix + kIncLaneKeyMax +
                      ramcrc_increment::kValueBytes < 0x100,
              "a lane's object has one length byte");
static_assert(kWrCounts + kIncKinds <= kWrHeadWords, "the head line holds the counts");
static_assert(sizeof(ramcrc_increment_arg) == 16 && sizeof(ramcrc_increment_summary) == 144 &&
                  ramcrc_increment::kPartBytes == 20, "increment ABI");
// (a key has at most 65,535 bytes, the width of the record's key length)
static_assert(ramcrc_increment::kStatusInvalidObject < kWrReach, "the record's status byte");

struct IncDesc {
    const uint64_t* args;                 // two words a request: add_int64, add_double
    uint64_t* bits;                       // scratch [nq]: the new value
    ramcrc_increment_summary* summary;
};

// -------------------------------------------------------------- k_inc_size
// w: the write's descriptor with the key buffer as its data, the requests the
// remove's, `group` one word a slot (k_rm_group's) and `summary` in scratch.
// q: the lookup over the caller's requests, its given hashes the group pass's.
__global__ __launch_bounds__(kPartThreads) void k_inc_size(RtabDesc a, LookDesc q, WrDesc w, IncDesc x)
{
    namespace rr = ramcrc_read;
    namespace rw = ramcrc_write;
    namespace ri = ramcrc_increment;
    if (rtab_refused(a))
        return;
    __shared__ unsigned long long red[kPartThreads / kWaveSize][5];
    const uint64_t ntiles = (w.nq + kPartThreads - 1) / kPartThreads;
    const uint32_t lane = threadIdx.x & (kWaveSize - 1), wv = threadIdx.x / kWaveSize;
    uint32_t cnt[kIncKinds] = {};   // (a lane takes fewer than 2^32 requests)
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i = tile * kPartThreads + threadIdx.x;
        uint64_t sums[5] = {0, 0, 0, 0, 0};   // bytes, counts, value, key, tombstone bytes
        uint32_t kind = kIncKinds;            // (counted by the scan, or no request)
        if (i < w.nq) {
            const uint64_t slot = w.slot[i];
            ramcrc_lookup_result res = ramcrc_look::no_result(RAMCRC_LOOKUP_BAD_KEY);
            uint64_t flags = 0, vd = 0, seg = 0, bits = 0;
            uint32_t st = rr::kStatusFormatError;
            kind = 3;
            if (slot != kResNone) {
                LookHit hit{0ull, 0u, ramcrc_look::Value{0u, 0u}};
                res = rtab_probe<true>(a, q, i, &hit);
                if (~w.group[slot] != i) {
                    st = rw::kStatusRetry;
                    kind = 4;
                } else {
                    const bool found = res.kind == RAMCRC_LOOKUP_OBJECT;
                    rr::Rules ru = rr::no_rules();
                    if (w.rules)
                        ru = rr::Rules{w.rules[2 * i], w.rules[2 * i + 1]};
                    const ri::Outcome o = ri::outcome(res.kind, res.version, found ? res.value_len : 0u, ru);
                    const bool obj = o.cur != 0;
                    st = o.status;
                    kind = st == rr::kStatusDoesntExist ? 0u : st == rr::kStatusExists ? 1u
                           : st == rr::kStatusWrongVersion ? 2u : 5u;
                    if (obj)
                        flags |= kWrTomb;   // (the replaced object's version: the tombstone's, and a rejected part's)
                    if (o.reach) {
                        bits = ri::sum(found ? part_bytes(hit.pay + hit.v.off, ri::kValueBytes) : 0ull,
                                       x.args[2 * i], x.args[2 * i + 1]);
                        const uint32_t kl = uint32_t(w.reqs[3 * i + 2]), dl = ri::image_len(kl);
                        flags |= kWrReach | (obj ? 0ull : kWrAlloc) |
                                 (res.kind == RAMCRC_LOOKUP_TOMBSTONE ? kWrOverTomb : 0ull) |
                                 (uint64_t(kl) << kWrKeyLenShift);
                        vd = ri::kValueBytes | (uint64_t(dl) << 32);
                        if (obj && w.batch_seg)
                            seg = w.batch_seg[res.ref.batch] + res.segment;
                        sums[0] = wr_posted(wr_size_of(flags, dl), w.cap);
                        sums[1] = 1ull | (obj ? 1ull << kWrCountBits : 1ull << (2 * kWrCountBits)) |
                                  (uint64_t(wr_meta_of(flags, dl)) << (3 * kWrCountBits));
                        sums[2] = ri::kValueBytes;
                        sums[3] = dl - ri::kValueBytes;
                        sums[4] = obj ? rw::kTombHeader + kl : 0u;
                        kind = kIncKinds;
                    }
                }
            }
            if (q.results)
                look_store(q, i, res);
            uint64_t* const rec = w.rec + 4 * i;
            rec[0] = res.version;
            rec[1] = vd;
            rec[2] = seg;
            rec[3] = flags | st;
            x.bits[i] = bits;
        }
        // the tile's sums: this workgroup alone has the tile
#pragma unroll
        for (uint32_t k = 0; k < 5; k++) {
            unsigned long long v = sums[k];
#pragma unroll
            for (int d = 1; d < kWaveSize; d <<= 1)
                v += __shfl_xor(v, d);
            if (lane == 0)
                red[wv][k] = v;
        }
        __syncthreads();
        if (threadIdx.x < 5) {
            const uint32_t k = threadIdx.x;
            unsigned long long v = red[0][k];
#pragma unroll
            for (uint32_t y = 1; y < kPartThreads / kWaveSize; y++)
                v += red[y][k];
            w.tile[kWrTileWords * tile + k] = v;
        }
        __syncthreads();   // red is free again
        // the outcomes no cut changes
#pragma unroll
        for (uint32_t k = 0; k < kIncKinds; k++)
            cnt[k] += kind == k;
    }
#pragma unroll
    for (uint32_t k = 0; k < kIncKinds; k++) {
        const unsigned long long n = rtab_block_sum(cnt[k], reinterpret_cast<uint64_t*>(&red[0][0]));
        if (threadIdx.x == 0 && n)
            atomicAdd(&w.head[kWrCounts + k], n);
    }
}

// -------------------------------------------------------------- k_inc_emit
// One object by 8 lanes (this one is `sub`), wr_tombstone's way: the message is
// the payload's bytes [4, end) -- 20 header bytes, the image's prefix, the key,
// the new value (increment_rules.h's object_byte) --; lane `sub` takes the
// sub-th eighth of it through the byte table, stores what it takes, moves its
// part to the end of the message and the group XORs the parts.  Every store
// lies inside the payload.
__device__ __forceinline__ void inc_object(uint64_t key, uint64_t pay, uint32_t klen, uint32_t sub,
                                           uint32_t ts, uint64_t version, uint64_t table_id, uint64_t bits,
                                           const uint32_t* t0)
{
    namespace ri = ramcrc_increment;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    const uint32_t M = ramcrc_write::kObjHeader - 4 + ri::image_len(klen);
    const uint32_t C = (M + kSlLanes - 1) / kSlLanes;
    const uint32_t lo = sub * C < M ? sub * C : M;
    const uint32_t hi = lo + C < M ? lo + C : M;
    const auto key_byte = [key](uint32_t k) { return uint32_t(*reinterpret_cast<const gu8*>(key + k)); };
    uint32_t c = sub == 0 ? 0xFFFFFFFFu : 0u;   // a fresh Crc32C in front of the first part
    for (uint32_t m = lo; m < hi; m++) {
        const uint32_t v = ri::object_byte(m, klen, ts, version, table_id, bits, key_byte);
        *reinterpret_cast<gw8*>(pay + 4 + m) = uint8_t(v);
        c = t0[(c ^ v) & 0xFF] ^ (c >> 8);
    }
    if (hi < M)
        c = mulmod_dev(c, sl_xpow8(M - hi));
    c ^= __shfl_xor(c, 1);
    c ^= __shfl_xor(c, 2);
    c ^= __shfl_xor(c, 4);
    const uint32_t ck = ~c;
    if (sub < 4)
        *reinterpret_cast<gw8*>(pay + sub) = uint8_t(ck >> (8 * sub));
}

// One object of a key of at most kIncLaneKeyMax bytes, by one lane: the whole
// entry at e (any residue) -- two metadata bytes, the 24 header bytes with the
// checksum, the image's prefix, the key, the new value.  The key is read once,
// as aligned 16-byte words; everything else comes from registers; the entry's
// 37 + klen bytes are stored by lane_store_entry.  The value lies klen bytes
// into the image's tail, at any byte of a word: it is shifted into the key's
// words by a shift the lane computes, the words it lands in chosen by
// predicates, so that every array index is a constant.
__device__ __forceinline__ void inc_object_lane(uint64_t e, uint64_t key, uint32_t klen, uint32_t meta,
                                                uint32_t ts, uint64_t version, uint64_t table_id,
                                                uint64_t bits, const uint32_t* t0)
{
    namespace ri = ramcrc_increment;
    constexpr uint32_t kTw = (kIncLaneKeyMax + ri::kValueBytes + 7) / 8;      // the tail: the key, then the value
    constexpr uint32_t kHead = 2 + ramcrc_write::kObjHeader + ri::kImagePrefix;   // 29 bytes in front of the key
    constexpr uint32_t kMax = kHead + kIncLaneKeyMax + ri::kValueBytes;
    constexpr uint32_t kWords = (kMax + 3) / 4;
    static_assert(kHead == 29 && kWords % 2 == 1, "three words and five bytes; an odd word count leaves a word of zeros");
    uint64_t tw[kTw + 1];
#pragma unroll
    for (uint32_t j = 0; j < kTw; j++) {
        tw[j] = 0;
        if (8 * j < klen)
            tw[j] = part_bytes(key + 8 * j, klen - 8 * j < 8 ? klen - 8 * j : 8u);
    }
    tw[kTw] = 0;
    const uint32_t vw = klen >> 3, vs = (klen & 7u) * 8;
#pragma unroll
    for (uint32_t j = 0; j <= kTw; j++) {
        if (j == vw)
            tw[j] |= bits << vs;
        if (j == vw + 1 && vs)
            tw[j] |= bits >> (64 - vs);
    }
    // the entry as 64-bit words, the checksum's four bytes still 0
    uint64_t x[kWords / 2 + 1];
    x[0] = meta | (uint64_t(ts) << 48);
    x[1] = (ts >> 16) | (version << 16);
    x[2] = (version >> 48) | (table_id << 16);
    x[3] = (table_id >> 48) | (uint64_t(ri::image_prefix_byte(0, klen)) << 16) |
           (uint64_t(ri::image_prefix_byte(1, klen)) << 24) | (uint64_t(ri::image_prefix_byte(2, klen)) << 32) |
           (tw[0] << 40);
#pragma unroll
    for (uint32_t j = 1; j <= kTw; j++)
        x[3 + j] = (tw[j - 1] >> 24) | (tw[j] << 40);
    static_assert(3 + kTw == kWords / 2, "the words of the longest entry, the last one zeros from its fifth byte on");
    const uint32_t size = kHead + klen + ri::kValueBytes;
    // Object::computeChecksum: the payload from its fifth byte on
    uint32_t c = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t b = 6; b < kMax; b++)
        if (b < size)
            c = t0[(c ^ uint32_t(x[b >> 3] >> (8 * (b & 7)))) & 0xFF] ^ (c >> 8);
    x[0] |= uint64_t(~c) << 16;
    lane_store_entry<kWords>(e, x, size);
}

__global__ __launch_bounds__(kPartThreads) void k_inc_emit(RtabDesc a, WrDesc w, IncDesc x)
{
    namespace rr = ramcrc_read;
    namespace rw = ramcrc_write;
    namespace ri = ramcrc_increment;
    typedef __attribute__((address_space(1))) uint8_t gw8;
    static_assert(kSlLanes == 8, "groups of 8 lanes");
    __shared__ uint32_t t0[256];
    __shared__ uint64_t wsum[kPartThreads / kWaveSize];
    // the long keys of a tile, as they come; sobj, stomb: payloads; stomb 0: none
    __shared__ uint64_t skey[kPartThreads], sobj[kPartThreads], stomb[kPartThreads];
    __shared__ uint64_t sver[kPartThreads], scur[kPartThreads], sseg[kPartThreads], stid[kPartThreads];
    __shared__ uint64_t sbits[kPartThreads];
    __shared__ uint32_t slen[kPartThreads];
    __shared__ uint32_t nlong;
    __shared__ uint32_t red[kPartThreads / kWaveSize];
    const uint32_t t = threadIdx.x;
    if (rtab_refused(a)) {
        if (blockIdx.x == 0 && t == 0) {
            ramcrc_increment_summary sm{};
            sm.spoiled = 1;
            *x.summary = sm;
        }
        return;
    }
    static_assert(kPartThreads == 256, "one byte-table entry per thread");
    t0[t] = g_tab.t0.t[t];
    const uint64_t ntiles = (w.nq + kPartThreads - 1) / kPartThreads;
    const uint64_t meta_all = w.head[kWrMeta];
    uint32_t cert = 0;   // thread 0: this workgroup's tiles, moved to the end of the metadata
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();   // the table is filled; the previous tile's groups have read their descriptors
        if (t == 0)
            nlong = 0;
        const uint64_t i = tile * kPartThreads + t;
        uint64_t flags = 0, wver = 0, vd = 0, seg = 0, size = 0, table_id = 0, key = 0, bits = 0;
        uint32_t dl = 0;
        if (i < w.nq) {
            const uint64_t* const rec = w.rec + 4 * i;
            wver = rec[0];
            vd = rec[1];
            seg = rec[2];
            flags = rec[3];
            dl = uint32_t(vd >> 32);
            if (flags & kWrReach) {
                size = wr_size_of(flags, dl);
                table_id = w.reqs[3 * i];
                key = w.data + w.reqs[3 * i + 1];
                bits = x.bits[i];
            }
        }
        const uint64_t* const ts = w.tile + kWrTileWords * tile;
        uint64_t tot;
        const uint64_t off = ts[0] + part_block_excl(wr_posted(size, w.cap), wsum, &tot);
        // (the scan cut where the entries stop fitting; checked here from the
        // same sums, as the last thing between a stale word and a stray store)
        const bool reach = (flags & kWrReach) != 0, in = reach && off + size <= w.cap;
        const uint32_t meta = in ? wr_meta_of(flags, dl) : 0u;
        const uint64_t ex2 =
            ts[5] + part_block_excl(((flags & kWrAlloc) ? 1ull : 0ull) | (uint64_t(meta) << 32), wsum, &tot);
        const uint32_t tile_meta = uint32_t(tot >> 32);
        const bool tomb = (flags & kWrTomb) != 0;
        const uint64_t cur = tomb ? wver : 0ull;
        const uint32_t klen = uint32_t(flags >> kWrKeyLenShift) & 0xFFFFu;
        uint64_t version = 0;
        uint32_t piece = 0;
        if (reach) {
            const uint64_t an = w.next_version + (ex2 & 0xFFFFFFFFull);
            version = rw::new_version(cur, (flags & kWrOverTomb) != 0, wver, an);
            if (cur == 0 && version != an)
                atomicMax(&w.head[kWrTop], static_cast<unsigned long long>(version + 1));
        }
        if (i < w.nq) {
            const uint32_t st = uint32_t(flags & 0xFF);
            const uint32_t status = !reach ? st : in ? rr::kStatusOk : rw::kStatusRetry;
            const uint64_t pv = in ? version : (st == rr::kStatusFormatError || st == rw::kStatusRetry) ? 0ull : cur;
            const uint64_t third = ri::part_value(status, bits, x.args[2 * i + 1]);
            uint32_t* const p = w.parts + 5 * i;
            p[0] = status;
            p[1] = uint32_t(pv);
            p[2] = uint32_t(pv >> 32);
            p[3] = uint32_t(third);
            p[4] = uint32_t(third >> 32);
        }
        uint2 ref = make_uint2(rw::kNone, rw::kNone);
        if (in) {
            // the entries' metadata, and its checksum moved to the end of the tile's metadata
            const uint32_t olen = rw::kObjHeader + dl;
            uint32_t nmo, nmt = 0;
            const uint64_t mo = rw::entry_meta(RAMCRC_LOG_ENTRY_TYPE_OBJ, olen, &nmo);
            const uint64_t eo = w.out + off, et = eo + nmo + olen;
            uint64_t mt = 0;
            uint32_t c = 0;
            ref.x = uint32_t(off);
            for (uint32_t b = 0; b < nmo; b++)
                c = t0[(c ^ uint32_t(mo >> (8 * b))) & 0xFF] ^ (c >> 8);
            if (tomb) {
                mt = rw::entry_meta(RAMCRC_LOG_ENTRY_TYPE_OBJTOMB, rw::kTombHeader + klen, &nmt);
                ref.y = uint32_t(et - w.out);
                for (uint32_t b = 0; b < nmt; b++)
                    c = t0[(c ^ uint32_t(mt >> (8 * b))) & 0xFF] ^ (c >> 8);
            }
            const uint32_t behind = tile_meta - uint32_t(ex2 >> 32) + uint32_t(ts[5] >> 32) - meta;
            piece = behind ? mulmod_dev(c, sl_xpow8(behind)) : c;
            if (klen <= kIncLaneKeyMax) {
                // (two metadata bytes each: the static_assert above, and kRmLaneKeyMax's)
                inc_object_lane(eo, key, klen, uint32_t(mo), w.timestamp, version, table_id, bits, t0);
                if (tomb)
                    rm_tombstone_lane(et, key, klen, uint32_t(mt), table_id, seg, cur, w.timestamp, t0);
            } else {
                for (uint32_t b = 0; b < nmo; b++)
                    *reinterpret_cast<gw8*>(eo + b) = uint8_t(mo >> (8 * b));
                for (uint32_t b = 0; b < nmt; b++)
                    *reinterpret_cast<gw8*>(et + b) = uint8_t(mt >> (8 * b));
                const uint32_t k = atomicAdd(&nlong, 1u);
                skey[k] = key;
                sobj[k] = eo + nmo;
                stomb[k] = tomb ? et + nmt : 0ull;
                sver[k] = version;
                scur[k] = cur;
                sseg[k] = seg;
                stid[k] = table_id;
                sbits[k] = bits;
                slen[k] = klen;
            }
        }
        if (w.refs && i < w.nq)
            w.refs[i] = ref;
        // the tile's metadata checksum, moved to the end of all metadata
#pragma unroll
        for (int d = 1; d < kWaveSize; d <<= 1)
            piece ^= __shfl_xor(piece, d);
        if ((t & (kWaveSize - 1)) == 0)
            red[t / kWaveSize] = piece;
        __syncthreads();
        if (t == 0) {
            uint32_t c = 0;
#pragma unroll
            for (uint32_t k = 0; k < kPartThreads / kWaveSize; k++)
                c ^= red[k];
            if (c) {
                const uint32_t behind = uint32_t(meta_all) - uint32_t(ts[5] >> 32) - tile_meta;
                cert ^= behind ? mulmod_dev(c, sl_xpow8(behind)) : c;
            }
        }
        const uint32_t nl = nlong, g = t / kSlLanes, sub = t % kSlLanes;
        for (uint32_t j = g; j < nl; j += kPartThreads / kSlLanes) {
            inc_object(skey[j], sobj[j], slen[j], sub, w.timestamp, sver[j], stid[j], sbits[j], t0);
            if (stomb[j])
                wr_tombstone(skey[j], stomb[j], slen[j], sub, stid[j], sseg[j], scur[j], w.timestamp, t0);
        }
    }
    __syncthreads();   // the table is filled, for a workgroup without a tile too
    // the certificate: every workgroup folds its share, the last one seals it
    if (t == 0) {
        if (cert)
            atomicXor(reinterpret_cast<unsigned int*>(&w.head[kWrCert]), cert);
        __threadfence();
        if (atomicAdd(&w.head[kWrTicket], 1ull) + 1 == gridDim.x) {
            __threadfence();
            const uint32_t folded = atomicXor(reinterpret_cast<unsigned int*>(&w.head[kWrCert]), 0u);
            const uint32_t head = uint32_t(w.head[kWrBytes]);
            // Segment::getAppendedLength: a fresh Crc32C moved behind the
            // metadata, the entries' metadata, the 4 head bytes, finalized
            uint32_t c = folded ^ (meta_all ? mulmod_dev(0xFFFFFFFFu, sl_xpow8(uint32_t(meta_all))) : 0xFFFFFFFFu);
            for (int b = 0; b < 4; b++)
                c = t0[(c ^ (head >> (8 * b))) & 0xFF] ^ (c >> 8);
            *w.cert = ramcrc_seg_cert{head, ~c};
            // the caller's summary from k_wr_scan's
            const unsigned long long top = atomicMax(&w.head[kWrTop], 0ull);
            const ramcrc_write_summary ws = *w.summary;
            ramcrc_increment_summary sm{};
            sm.ok = ws.ok;
            sm.created = ws.ok - ws.tombstones;
            sm.doesnt_exist = ws.doesnt_exist;
            sm.object_exists = ws.object_exists;
            sm.wrong_version = ws.wrong_version;
            sm.invalid_object = w.head[kWrCounts + 5];
            sm.bad = ws.bad;
            sm.retry_duplicate = ws.retry_duplicate;
            sm.retry_full = ws.retry_full;
            sm.tombstones = ws.tombstones;
            sm.allocated = ws.allocated;
            sm.next_version = top > ws.next_version ? top : ws.next_version;
            sm.out_bytes = ws.out_bytes;
            sm.object_bytes = ws.object_bytes;
            sm.tombstone_bytes = ws.tombstone_bytes;
            sm.value_bytes = ws.value_bytes;
            sm.key_bytes = ws.key_bytes;
            *x.summary = sm;
        }
    }
}

}  // namespace
