// MI355X (gfx950) kernels for batched CRC32C, plus the device half of the C ABI.
//
// What is computed: for every buffer i, the state RAMCloud's
// Crc32C::update(buf_i, len_i) (src/Crc32C.h:200-206) reaches from state
// init[i] (default 0xFFFFFFFF, src/Crc32C.h:177), optionally inverted as by
// getResult() (src/Crc32C.h:247-249).  Bit-identical to intelCrc32C /
// softwareCrc32C (src/Crc32C.h:39-153).
//
// How (see DESIGN.md for the derivation and the roofline):
//
//  * CRC is linear over GF(2) and every operator is a multiplication by a
//    constant power of x (gf2.h), so a buffer can be cut anywhere, the pieces
//    CRC'd from state 0, and the partials shifted into place and XORed.
//  * k_chunks -- the byte scan.  Buffers >= 64 KiB are cut into 256 KiB
//    chunks aligned to absolute 256 KiB boundaries; one wave scans one chunk
//    as 1 KiB blocks (lane l owns bytes [16l, 16l+16) of every block: one
//    coalesced global_load_dwordx4 per lane per block).  Each lane keeps four
//    accumulators (one per dword) updated by Horner's rule
//        u <- X^1024(u) ^ w
//    so the only per-byte work is one X^1024 table lookup per input byte.
//    The four X^1024 byte tables live in LDS replicated 32 times so that
//    lane l always hits bank l%32: ds_read_b32 without bank conflicts.  The
//    LDS address of a lookup is formed by ONE v_perm_b32 (byte k of u into
//    address byte 1, the lane's bank offset into byte 0, the table pair into
//    byte 2).  At the end of a chunk the 256 accumulators are folded with
//    X^4 in-lane and X^16..X^512 across lanes (wave shuffles), giving the raw
//    CRC of the chunk relative to its 1 KiB-aligned end.
//  * k_combine -- one wave per buffer merges its chunk partials with
//    x^(8d) constants (4 table lookups + GF(2) multiplies), removes the
//    zero-padding of the last block with x^(-8p), and writes the result.
//    The initial state is injected as an XOR into the first four message
//    bytes (raw(s,M) = raw(0, M ^ s||0...)) inside k_chunks.
//  * k_bin_* / k_entries -- small buffers (log entries, objects): binned by
//    128-byte step count, then a group of 8 lanes per entry; entries of one
//    window take the tiny phase (one position-table lookup per byte), longer
//    ones Horner with X^128.
//  * k_plan_* -- for the general offset/length table: per-entry chunk counts
//    and their exclusive prefix so waves can map a global chunk index to
//    (entry, chunk) with two binary searches.
//  * k_seg_walk / k_walk_* -- Segment::checkMetadataIntegrity over whole
//    segments, and the records the replay checks read.
//  * k_app_* -- walked records appended into per-partition recovery segments,
//    with their certificates.
//  * k_res_* -- which replayed objects and tombstones a recovery master keeps
//    (DESIGN.md 5.10).
//  * k_rtab_* -- the same decision batch by batch, in a table that outlives
//    the call.
//
// The kernels live in per-family parts included below, in this order, into
// this one translation unit (shared __device__ tables and LDS layouts, no
// relocatable device code):
//   dev_common.inc   geometry, tables, LDS layouts, operators, descriptors
//   dev_chunks.inc   k_chunks, k_combine
//   dev_bins.inc     small-entry configuration, k_bin_count/_scatter/_one
//   dev_entries.inc  k_entries (tiny, multi-window and long phases)
//   dev_plan.inc     k_plan_count, k_plan_scan, status kernels
//   dev_host.inc     ramcrc_ctx and the host launch helpers
//   dev_walk.inc     k_seg_walk and the parallel walk (k_walk_*)
//   dev_checks.inc   k_obj_compare, k_obj_stamp, certificate kernels
//   dev_append.inc   k_app_mark, k_app_scan, k_app_copy (recovery-segment append)
//   dev_sidelog.inc  k_sl_stamp (rewritten tombstones, references, counts)
//   dev_partition.inc  k_part_* (key hash, tablet lookup, liveness: the placement list)
//   dev_resolve.inc  k_res_* (replayed objects and tombstones: newest wins)
//   dev_replay_table.inc  k_rtab_* (newest wins across batches: the persistent table,
//                         its lookup by key and a multi-read's reply)
//   dev_read_hashes.inc   k_rh_* (an indexed read's reply: objects by primary-key hash)
//   dev_enumerate.inc     k_en_* (one reply of a table enumeration: a walk over the buckets)
//   dev_index.inc         k_ix_*, k_ixl_* (a secondary index: sorted entries and range lookups)
//   dev_migrate.inc       k_mig_* (a tablet migration: filtered log-order scan into transfer segments)
// This file keeps the extern "C" entry points of include/ramcrc.h.
//
// No MFMA: this is a byte scan, bound by HBM reads.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <mutex>
#include <new>
#include <utility>
#include <vector>
#include <stdio.h>
#include <string.h>

#include "gf2.h"
#include "walk_rules.h"
#include "murmur3.h"
#include "partition_rules.h"
#include "lookup_rules.h"
#include "read_rules.h"
#include "read_hashes_rules.h"
#include "enumerate_rules.h"
#include "index_rules.h"
#include "resolve_rules.h"
#include "sidelog_rules.h"
#include "write_rules.h"
#include "remove_rules.h"
#include "increment_rules.h"
#include "clean_rules.h"
#include "migrate_rules.h"
#include "ramcrc.h"

namespace {

using namespace ramcrc_walk;   // Hop, hop_of, plausible, first_hop4, kNumTypes

using ramcrc::OpTable;

}  // namespace

#include "dev_common.inc"
#include "dev_chunks.inc"
#include "dev_bins.inc"
#include "dev_entries.inc"
#include "dev_plan.inc"
#include "dev_host.inc"
#include "dev_walk.inc"
#include "dev_checks.inc"
#include "dev_append.inc"
#include "dev_sidelog.inc"
#include "dev_partition.inc"
#include "dev_resolve.inc"
#include "dev_replay_table.inc"
#include "dev_read_hashes.inc"
#include "dev_enumerate.inc"
#include "dev_index.inc"
#include "dev_write.inc"
#include "dev_remove.inc"
#include "dev_increment.inc"
#include "dev_clean.inc"
#include "dev_migrate.inc"

extern "C" {

int ramcrc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int ramcrc_last_hip_error(void) { return t_last_hip; }

const char* ramcrc_strerror(int code)
{
    switch (code) {
    case RAMCRC_OK: return "ok";
    case RAMCRC_EINVAL: return "invalid argument";
    case RAMCRC_ENOMEM: return "out of memory";
    case RAMCRC_EHIP: return hipGetErrorString(hipError_t(t_last_hip));
    case RAMCRC_ENODEV: return "no usable device";
    case RAMCRC_ERCCL: return "rccl failure";
    case RAMCRC_EREFUSED: return "launch refused: chunk scratch too small (ramcrc_ctx_reserve), or a placement list refused";
    case RAMCRC_EINTERNAL: return "launch refused: inconsistent small-entry bin layout";
    case RAMCRC_EPEER: return "another rank of the shard failed this step";
    default: return "unknown error";
    }
}

#ifndef RAMCRC_SRC_SHA
#define RAMCRC_SRC_SHA "unknown"
#endif
#ifndef RAMCRC_DEFINES
#define RAMCRC_DEFINES "none"   // build.py: the -D knobs of a variant build (variants.py)
#endif
#define RAMCRC_STR2(x) #x
#define RAMCRC_STR(x) RAMCRC_STR2(x)

// Probe builds only: copies k_entries' phase stamps (RAMCRC_STAMPS) to host
// memory; RAMCRC_EINVAL in product builds.  Not part of the C ABI header.
int ramcrc_debug_stamps(void* out, uint64_t bytes)
{
#if RAMCRC_STAMPS
    if (bytes > sizeof(g_stamps))
        bytes = sizeof(g_stamps);
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), bytes) == hipSuccess ? RAMCRC_OK : RAMCRC_EHIP;
#else
    (void)out;
    (void)bytes;
    return RAMCRC_EINVAL;
#endif
}

const char* ramcrc_build_info(void)
{
    // src_sha: sha256 of the sources the library was built from (build.py),
    // the same marker build.py reads back to decide staleness
    return "ramcrc gfx950 src_sha=" RAMCRC_SRC_SHA
           " chunk=" RAMCRC_STR(RAMCRC_CHUNK_SHIFT) "..20 (adaptive: largest giving every wave two chunks)"
           " block=1KiB waves/WG=16 unroll=" RAMCRC_STR(RAMCRC_UNROLL)
           " lds_chunks=" RAMCRC_STR(RAMCRC_LDS_CHUNKS) " lds_entries=" RAMCRC_STR(RAMCRC_LDS_ENTRIES)
           " entries: waves=" RAMCRC_STR(RAMCRC_ENT_WAVES) " smallk=" RAMCRC_STR(RAMCRC_SMALLK)
           " pu=" RAMCRC_STR(RAMCRC_PU)
           " large_min=64KiB part_shift=" RAMCRC_STR(RAMCRC_PART_SHIFT)
           " defines=" RAMCRC_DEFINES;
}

int ramcrc_ctx_create(int device, ramcrc_ctx** out)
{
    if (!out)
        return RAMCRC_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return RAMCRC_ENODEV;
    DeviceGuard g(device);
    if (!g.ok)
        return RAMCRC_ENODEV;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "ramcrc: device %d is %s, this build targets gfx950 only\n", device,
                prop.gcnArchName);
        return RAMCRC_ENODEV;
    }
    ramcrc_ctx* c = new (std::nothrow) ramcrc_ctx();
    if (!c)
        return RAMCRC_ENOMEM;
    c->device = device;
    c->ncu = prop.multiProcessorCount;
    c->ncu_all = c->ncu;
    // four words: [0] the status bits, [1] k_status_take's copy for the host, [2..3] spare
    if (hipMalloc(reinterpret_cast<void**>(&c->status), 16) != hipSuccess) {
        delete c;
        return RAMCRC_ENOMEM;
    }
    (void)hipMemset(c->status, 0, 16);
    if (hipMalloc(reinterpret_cast<void**>(&c->bins), sizeof(BinTable)) != hipSuccess) {
        ramcrc_ctx_destroy(c);
        return RAMCRC_ENOMEM;
    }
    (void)hipMemset(c->bins, 0, sizeof(BinTable));   // hist must start at zero
    *out = c;
    return RAMCRC_OK;
}

int ramcrc_ctx_destroy(ramcrc_ctx* c)
{
    if (!c)
        return RAMCRC_OK;
    DeviceGuard g(c->device);
    (void)hipDeviceSynchronize();
    if (c->partials) (void)hipFree(c->partials);
    if (c->plan_local) (void)hipFree(c->plan_local);
    if (c->group_pref) (void)hipFree(c->group_pref);
    if (c->status) (void)hipFree(c->status);
    if (c->bins) (void)hipFree(c->bins);
    if (c->sdesc) (void)hipFree(c->sdesc);
    if (c->sidx) (void)hipFree(c->sidx);
    if (c->sinit) (void)hipFree(c->sinit);
    if (c->obj_out) (void)hipFree(c->obj_out);
    if (c->cert_scratch) (void)hipFree(c->cert_scratch);
    if (c->walk_parts) (void)hipFree(c->walk_parts);
    if (c->walk_fallback) (void)hipFree(c->walk_fallback);
    if (c->walk_base) (void)hipFree(c->walk_base);
    if (c->walk_recs) (void)hipFree(c->walk_recs);
    if (c->walk_pool) (void)hipFree(c->walk_pool);
    if (c->walk_pool_owner) (void)hipFree(c->walk_pool_owner);
    if (c->walk_blocks) (void)hipFree(c->walk_blocks);
    if (c->walk_pool_used) (void)hipFree(c->walk_pool_used);
    if (c->walk_sum) (void)hipFree(c->walk_sum);
    if (c->walk_left) (void)hipFree(c->walk_left);
    if (c->d_stage) (void)hipFree(c->d_stage);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->compute_stream) (void)hipStreamDestroy(c->compute_stream);
    for (auto& ev : c->ev_used) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    for (auto& ev : c->ev_free) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    delete c;
    return RAMCRC_OK;
}

int ramcrc_ctx_reserve(ramcrc_ctx* c, uint64_t max_chunks, uint64_t max_entries)
{
    if (!c)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    return reserve_locked(c, max_chunks, max_entries);
}

int ramcrc_debug_scratch_allocations(uint64_t* count)
{
    if (!count)
        return RAMCRC_EINVAL;
    *count = g_scratch_allocations.load(std::memory_order_relaxed);
    return RAMCRC_OK;
}

int ramcrc_ctx_set_option(ramcrc_ctx* c, int option, int64_t value)
{
    if (!c)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    switch (option) {
    case RAMCRC_OPT_SERIAL_WALK: c->serial_walk = value != 0; return RAMCRC_OK;
    case RAMCRC_OPT_TEST_FAIL_AFTER_COUNT:
        if (value < 0 || value > 1000)
            return RAMCRC_EINVAL;
        c->fail_after_count = int(value);
        return RAMCRC_OK;
    case RAMCRC_OPT_TEST_DIRTY_BINS:
        if (value < 0 || value > 0xFFFFFFFFll)
            return RAMCRC_EINVAL;
        c->dirty_bins = uint32_t(value);
        return RAMCRC_OK;
    case RAMCRC_OPT_TEST_BIN_STRAGGLER:
        c->bin_straggler = value != 0;
        return RAMCRC_OK;
    case RAMCRC_OPT_BIN_ONE:
        c->bin_one = value != 0;
        return RAMCRC_OK;
    case RAMCRC_OPT_VERIFY_IN_WALK:
        if (value < 0 || value > 2)
            return RAMCRC_EINVAL;
        c->verify_in_walk = int(value);
        return RAMCRC_OK;
    case RAMCRC_OPT_WALK_PART_SHIFT:
        if (value != 0 && (value < kPartShiftMin || value > 20))
            return RAMCRC_EINVAL;
        c->walk_pshift = uint32_t(value);
        return RAMCRC_OK;
    default: return RAMCRC_EINVAL;
    }
}

int ramcrc_ctx_set_timing(ramcrc_ctx* c, int enable)
{
    if (!c)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    c->timing = enable != 0;
    return RAMCRC_OK;
}

int ramcrc_stream_create_cu_mask(int device, const uint32_t* cu_mask, uint32_t mask_words,
                                 void** out_stream)
{
    if (!cu_mask || !out_stream || mask_words == 0 || mask_words > 8)
        return RAMCRC_EINVAL;
    DeviceGuard g(device);
    if (!g.ok)
        return RAMCRC_ENODEV;
    hipStream_t st = nullptr;
    HIPCHK(hipExtStreamCreateWithCUMask(&st, mask_words, cu_mask));
    *out_stream = st;
    return RAMCRC_OK;
}

int ramcrc_stream_destroy(void* stream)
{
    if (!stream)
        return RAMCRC_EINVAL;
    HIPCHK(hipStreamDestroy(reinterpret_cast<hipStream_t>(stream)));
    return RAMCRC_OK;
}

int ramcrc_ctx_set_cus(ramcrc_ctx* c, int ncu)
{
    if (!c || ncu < 0)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (ncu == 0 || ncu > c->ncu_all)
        ncu = c->ncu_all;
    c->ncu = ncu;
    return RAMCRC_OK;
}

int ramcrc_ctx_scan_time(ramcrc_ctx* c, double* total_ms, uint64_t* launches)
{
    if (!c)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    double sum = 0;
    uint64_t cnt = 0;
    for (auto& ev : c->ev_used) {
        HIPCHK(hipEventSynchronize(ev.second));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev.first, ev.second));
        sum += ms;
        cnt++;
        c->ev_free.push_back(ev);
    }
    c->ev_used.clear();
    if (total_ms)
        *total_ms = sum;
    if (launches)
        *launches = cnt;
    return RAMCRC_OK;
}

int ramcrc_ctx_debug_bins(ramcrc_ctx* c, uint64_t* host, uint64_t nwords, uint32_t* par_next)
{
    if (!c || !host)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    HIPCHK(hipDeviceSynchronize());
    // count[kNB], then cursor[0][kNB], cursor[1][kNB], then hist[0], hist[1] (as uint64),
    // the k_bin_one rescues
    std::vector<uint64_t> v;
    BinTable h;
    HIPCHK(hipMemcpy(&h, c->bins, sizeof(BinTable), hipMemcpyDeviceToHost));
    for (int b = 0; b < kNB; b++) v.push_back(h.count[b]);
    for (int p = 0; p < 2; p++)
        for (int b = 0; b < kNB; b++) v.push_back(h.ctr[p].cursor[b]);
    for (int p = 0; p < 2; p++)
        for (int b = 0; b < kNB; b++) v.push_back(h.ctr[p].hist[b]);
    v.push_back(h.rescues);
    for (uint64_t i = 0; i < nwords && i < v.size(); i++)
        host[i] = v[i];
    if (par_next)
        *par_next = c->bin_par;
    return RAMCRC_OK;
}

int ramcrc_ctx_status(ramcrc_ctx* c, uint32_t* status)
{
    if (!c || !status)
        return RAMCRC_EINVAL;
    DeviceGuard g(c->device);
    HIPCHK(hipMemcpy(status, c->status, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RAMCRC_OK;
}

int ramcrc_ctx_check(ramcrc_ctx* c, void* stream)
{
    if (!c)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIPCHK(hipStreamSynchronize(s));
    uint32_t st = 0;
    HIPCHK(hipMemcpy(&st, c->status, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (!(st & kStatusSticky))
        return RAMCRC_OK;
    // take the sticky bits with one device atomic: a bit another stream's
    // launch sets meanwhile is either taken here or stays for the next check
    hipLaunchKernelGGL(k_status_take, dim3(1), dim3(1), 0, s, c->status);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(&st, c->status + 1, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (st & kStatusBins)
        return RAMCRC_EINTERNAL;
    return (st & kStatusSticky) ? RAMCRC_EREFUSED : RAMCRC_OK;
}

int ramcrc_segments_device(ramcrc_ctx* c, const void* d_base, uint64_t seg_bytes, uint64_t nseg,
                           const uint32_t* d_init, uint32_t* d_out, uint32_t flags, void* stream)
{
    if (!c || !d_out || (!d_base && nseg && seg_bytes) || (flags & ~RAMCRC_FINALIZE))
        return RAMCRC_EINVAL;
    if (nseg == 0)
        return RAMCRC_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    BatchDesc d{};
    d.cshift = kChunkShift;
    d.base = static_cast<const uint8_t*>(d_base);
    d.seg_bytes = seg_bytes;
    d.n = nseg;
    d.init = d_init;
    d.out = d_out;
    d.flags = flags;
    if (seg_bytes < kLargeMin) {
        return launch_binned<kSegUniform>(c, d, s, 0);
    }
    const uint64_t B = reinterpret_cast<uint64_t>(d_base);
    if ((B % kChunk) == 0 && (seg_bytes % kChunk) == 0) {
        // The recovery-scan fast path: no plan, chunk g -> (g / per, g % per).
        // Largest chunk (256 KiB .. 1 MiB) that still gives every wave two
        // chunks: fewer per-chunk pipeline drains and folds.
        const uint64_t waves = uint64_t(c->ncu) * kWavesPerGroup;
        uint32_t shift = kChunkShift;
        while (shift < 20 && (B % (2ull << shift)) == 0 && (seg_bytes % (2ull << shift)) == 0 &&
               (seg_bytes >> (shift + 1)) * nseg >= 2 * waves)
            shift++;
        d.cshift = shift;
        const uint64_t per = seg_bytes >> shift;
        int rc = reserve_locked(c, per * nseg, 1);
        if (rc)
            return rc;
        Plan pl = make_plan(c, 0);
        {
            ScanTimer t(c, s);
            t.launch(k_chunks<kSegAligned>, dim3(c->ncu), dim3(kThreads), d, pl, per);
        }
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL((k_combine<kSegAligned, false>), dim3((nseg + 3) / 4), dim3(256), 0, s,
                           d, pl, per);
        HIPCHK(hipGetLastError());
        return RAMCRC_OK;
    }
    int rc = reserve_locked(c, nseg * (seg_bytes / kChunk + 2) + 16, nseg);
    if (rc)
        return rc;
    return launch_planned<kSegUniform>(c, d, s);
}

int ramcrc_batch_device(ramcrc_ctx* c, const void* d_base, const uint64_t* d_off,
                        const uint64_t* d_len, const uint32_t* d_init, uint32_t* d_out, uint64_t n,
                        uint32_t flags, void* stream)
{
    if (flags & ~RAMCRC_FINALIZE)
        return RAMCRC_EINVAL;   // unknown flag bits (2 was the removed RAMCRC_ORDERED)
    if (n == 0)
        return c ? RAMCRC_OK : RAMCRC_EINVAL;
    if (!c || !d_out || !d_off || !d_len || !d_base)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    int rc = reserve_locked(c, default_chunk_bound(n), n);
    if (rc)
        return rc;
    BatchDesc d{};
    d.cshift = kChunkShift;
    d.base = static_cast<const uint8_t*>(d_base);
    d.off = d_off;
    d.len = d_len;
    d.n = n;
    d.init = d_init;
    d.out = d_out;
    d.flags = flags;
    return launch_planned<kTable>(c, d, reinterpret_cast<hipStream_t>(stream));
}

int ramcrc_entries_device(ramcrc_ctx* c, const void* d_base, const uint64_t* d_off,
                          const uint64_t* d_len, const uint32_t* d_init, uint32_t* d_out, uint64_t n,
                          uint32_t flags, void* stream)
{
    if (flags & ~RAMCRC_FINALIZE)
        return RAMCRC_EINVAL;   // unknown flag bits (2 was the removed RAMCRC_ORDERED)
    if (n == 0)
        return c ? RAMCRC_OK : RAMCRC_EINVAL;
    if (!c || !d_out || !d_off || !d_len || !d_base)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    BatchDesc d{};
    d.cshift = kChunkShift;
    d.base = static_cast<const uint8_t*>(d_base);
    d.off = d_off;
    d.len = d_len;
    d.n = n;
    d.init = d_init;
    d.out = d_out;
    d.flags = flags;
    return launch_binned<kTable>(c, d, s, 0);
}

int ramcrc_batch_host(ramcrc_ctx* c, const void* const* ptrs, const uint64_t* lens,
                      const uint32_t* init, uint32_t* out, uint64_t n, uint32_t flags)
{
    if (!c || (n && (!ptrs || !lens || !out)) || (flags & ~RAMCRC_FINALIZE))
        return RAMCRC_EINVAL;
    if (n == 0)
        return RAMCRC_OK;
    // The context lock is held from sizing the staging buffers to the final
    // synchronize: another thread on this context must not free or refill
    // them while they are being copied from.
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    // Pack every buffer 16-byte aligned into one pinned staging area, then one
    // H2D copy, one batch launch, one D2H copy.
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (lens[i] && !ptrs[i])
            return RAMCRC_EINVAL;
        total += (lens[i] + 15) & ~uint64_t(15);
    }
    const uint64_t meta = n * (2 * sizeof(uint64_t) + 2 * sizeof(uint32_t));
    const uint64_t need = total + meta + 64;
    if (c->h_stage_cap < need) {
        if (c->h_stage) (void)hipHostFree(c->h_stage);
        c->h_stage = nullptr;
        c->h_stage_cap = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&c->h_stage), need, hipHostMallocDefault) !=
            hipSuccess)
            return RAMCRC_ENOMEM;
        c->h_stage_cap = need;
    }
    if (c->d_stage_cap < need) {
        if (c->d_stage) (void)hipFree(c->d_stage);
        c->d_stage = nullptr;
        c->d_stage_cap = 0;
        if (hipMalloc(reinterpret_cast<void**>(&c->d_stage), need) != hipSuccess)
            return RAMCRC_ENOMEM;
        c->d_stage_cap = need;
    }
    if (!c->copy_stream)
        HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    uint8_t* h = c->h_stage;
    uint64_t* h_off = reinterpret_cast<uint64_t*>(h + total);
    uint64_t* h_len = h_off + n;
    uint32_t* h_init = reinterpret_cast<uint32_t*>(h_len + n);
    uint32_t* h_out = h_init + n;
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (lens[i])
            memcpy(h + pos, ptrs[i], lens[i]);
        h_off[i] = pos;
        h_len[i] = lens[i];
        h_init[i] = init ? init[i] : 0xFFFFFFFFu;
        pos += (lens[i] + 15) & ~uint64_t(15);
    }
    uint8_t* d = c->d_stage;
    hipStream_t s = c->copy_stream;
    const uint64_t in_bytes = total + n * (2 * sizeof(uint64_t) + sizeof(uint32_t));
    HIPCHK(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    uint64_t* d_off = reinterpret_cast<uint64_t*>(d + total);
    uint64_t* d_len = d_off + n;
    uint32_t* d_init = reinterpret_cast<uint32_t*>(d_len + n);
    uint32_t* d_out = d_init + n;
    int rc = ramcrc_batch_device(c, d, d_off, d_len, d_init, d_out, n, flags, s);
    if (rc) {
        (void)hipStreamSynchronize(s);   // the H2D copy reads h_stage
        return rc;
    }
    HIPCHK(hipMemcpyAsync(h_out, d_out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    rc = ramcrc_ctx_check(c, s);   // synchronizes s; a refused launch wrote nothing
    if (rc)
        return rc;
    memcpy(out, h_out, n * sizeof(uint32_t));
    return RAMCRC_OK;
}

int ramcrc_stream_host(ramcrc_ctx* c, const void* h_base, uint64_t seg_bytes, uint64_t nseg,
                       uint32_t* h_out, uint32_t flags, int batch, int depth)
{
    if (!c || !h_base || !h_out || batch < 1 || depth < 1 || seg_bytes == 0 ||
        (flags & ~RAMCRC_FINALIZE))
        return RAMCRC_EINVAL;
    if (nseg == 0)
        return RAMCRC_OK;
    std::lock_guard<std::recursive_mutex> lk(c->mu);   // held until both streams drained
    DeviceGuard g(c->device);
    if (depth > 8)
        depth = 8;
    const uint64_t slot_bytes = uint64_t(batch) * seg_bytes;
    // Each slot: batch*seg_bytes of data + batch CRCs.
    const uint64_t slot_stride = (slot_bytes + 4 * uint64_t(batch) + 4095) & ~uint64_t(4095);
    const uint64_t need = slot_stride * uint64_t(depth);
    if (c->d_stage_cap < need) {
        if (c->d_stage) (void)hipFree(c->d_stage);
        c->d_stage = nullptr;
        c->d_stage_cap = 0;
        if (hipMalloc(reinterpret_cast<void**>(&c->d_stage), need) != hipSuccess)
            return RAMCRC_ENOMEM;
        c->d_stage_cap = need;
    }
    if (!c->copy_stream)
        HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    if (!c->compute_stream)
        HIPCHK(hipStreamCreateWithFlags(&c->compute_stream, hipStreamNonBlocking));
    hipEvent_t copied[8] = {}, done[8] = {};
    int rc = RAMCRC_OK;
    auto hip = [&](hipError_t e) {
        if (e != hipSuccess && rc == RAMCRC_OK) {
            t_last_hip = int(e);
            rc = RAMCRC_EHIP;
        }
        return rc == RAMCRC_OK;
    };
    for (int k = 0; k < depth && rc == RAMCRC_OK; k++) {
        hip(hipEventCreateWithFlags(&copied[k], hipEventDisableTiming));
        hip(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
    }
    const uint8_t* src = static_cast<const uint8_t*>(h_base);
    const uint64_t nb = (nseg + batch - 1) / batch;
    // On any failure the loop stops issuing; the streams are drained below
    // before the events are destroyed and before returning, so no copy into
    // h_out or out of h_base is still in flight when the call returns.
    for (uint64_t b = 0; b < nb && rc == RAMCRC_OK; b++) {
        const int k = int(b % depth);
        const uint64_t first = b * batch;
        const uint64_t cnt = (nseg - first) < uint64_t(batch) ? (nseg - first) : uint64_t(batch);
        uint8_t* slot = c->d_stage + uint64_t(k) * slot_stride;
        uint32_t* slot_out = reinterpret_cast<uint32_t*>(slot + slot_bytes);
        if (b >= uint64_t(depth) && !hip(hipStreamWaitEvent(c->copy_stream, done[k], 0)))
            break;
        if (!hip(hipMemcpyAsync(slot, src + first * seg_bytes, cnt * seg_bytes,
                                hipMemcpyHostToDevice, c->copy_stream)) ||
            !hip(hipEventRecord(copied[k], c->copy_stream)) ||
            !hip(hipStreamWaitEvent(c->compute_stream, copied[k], 0)))
            break;
        rc = ramcrc_segments_device(c, slot, seg_bytes, cnt, nullptr, slot_out, flags,
                                    c->compute_stream);
        if (rc)
            break;
        if (!hip(hipMemcpyAsync(h_out + first, slot_out, cnt * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, c->compute_stream)) ||
            !hip(hipEventRecord(done[k], c->compute_stream)))
            break;
    }
    hip(hipStreamSynchronize(c->compute_stream));
    hip(hipStreamSynchronize(c->copy_stream));
    for (int k = 0; k < depth; k++) {
        if (copied[k]) (void)hipEventDestroy(copied[k]);
        if (done[k]) (void)hipEventDestroy(done[k]);
    }
    return rc;
}


namespace {
int walk_impl(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride, uint32_t seg_capacity,
              uint64_t n_seg, const ramcrc_seg_cert* d_certs, ramcrc_seg_status* d_status,
              ramcrc_seg_entry* d_entries, uint64_t entries_cap, uint64_t* d_n_entries,
              hipStream_t s, uint32_t* sum, uint32_t* d_obj_crc = nullptr);
int verify_impl(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride,
                const ramcrc_seg_entry* d_entries, uint64_t entries_cap, const uint64_t* d_n_entries,
                uint32_t* d_obj_crc, ramcrc_seg_status* d_status, hipStream_t s, const uint32_t* sum,
                uint64_t n_seg = 0);
}  // namespace

int ramcrc_segment_walk_device(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride,
                               uint32_t seg_capacity, uint64_t n_seg,
                               const ramcrc_seg_cert* d_certs, ramcrc_seg_status* d_status,
                               ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                               uint64_t* d_n_entries, void* stream)
{
    if (!c)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    return walk_impl(c, d_base, seg_stride, seg_capacity, n_seg, d_certs, d_status, d_entries,
                     entries_cap, d_n_entries, reinterpret_cast<hipStream_t>(stream), nullptr);
}

int ramcrc_replay_verify_device(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride,
                                uint32_t seg_capacity, uint64_t n_seg, const ramcrc_seg_cert* d_certs,
                                ramcrc_seg_status* d_status, ramcrc_seg_entry* d_entries,
                                uint64_t entries_cap, uint64_t* d_n_entries, uint32_t* d_obj_crc,
                                void* stream)
{
    if (!c)
        return RAMCRC_EINVAL;
    if (entries_cap && !d_obj_crc)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc = grow_device(reinterpret_cast<void**>(&c->walk_sum), &c->walk_sum_cap, 4, sizeof(uint32_t));
    if (rc)
        return rc;
    rc = walk_impl(c, d_base, seg_stride, seg_capacity, n_seg, d_certs, d_status, d_entries,
                   entries_cap, d_n_entries, s, c->walk_sum,
                   entries_cap && c->verify_in_walk ? d_obj_crc : nullptr);
    if (rc || n_seg == 0)
        return rc;
    return verify_impl(c, d_base, seg_stride, d_entries, entries_cap, d_n_entries, d_obj_crc,
                       d_status, s, c->walk_sum, n_seg);
}

namespace {
int walk_impl(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride, uint32_t seg_capacity,
              uint64_t n_seg, const ramcrc_seg_cert* d_certs, ramcrc_seg_status* d_status,
              ramcrc_seg_entry* d_entries, uint64_t entries_cap, uint64_t* d_n_entries,
              hipStream_t s, uint32_t* sum, uint32_t* d_obj_crc)
{
    if (!d_n_entries || (entries_cap && !d_entries))
        return RAMCRC_EINVAL;
    if (n_seg && (!d_base || !d_certs || !d_status))
        return RAMCRC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_base) & 15) || (seg_stride & 15) || (seg_capacity & 15) ||
        n_seg > 0xFFFFFFFFull || (n_seg > 1 && seg_stride < seg_capacity))
        return RAMCRC_EINVAL;
    if (n_seg == 0 || c->serial_walk) {
        // (the parallel walk's k_walk_probe zeroes these)
        HIPCHK(hipMemsetAsync(d_n_entries, 0, sizeof(uint64_t), s));
        if (sum)
            HIPCHK(hipMemsetAsync(sum, 0, sizeof(uint32_t), s));
    }
    if (n_seg == 0)
        return RAMCRC_OK;
    WalkDesc w{};
    w.base = static_cast<const uint8_t*>(d_base);
    w.stride = seg_stride;
    w.capacity = seg_capacity;
    w.nseg = n_seg;
    w.certs = d_certs;
    w.status = d_status;
    w.entries = reinterpret_cast<u32x4*>(d_entries);
    w.cap = entries_cap;
    w.n_entries = reinterpret_cast<unsigned long long*>(d_n_entries);
    w.only = nullptr;
    w.sum = sum;
    {
        int rc0 = grow_device(reinterpret_cast<void**>(&c->walk_base), &c->walk_base_cap, n_seg,
                              sizeof(uint64_t));
        if (rc0)
            return rc0;
    }
    w.seg_base = c->walk_base;   // every segment's first record slot (both walkers)
    uint64_t grid = n_seg;
    if (grid > uint64_t(64) * c->ncu)
        grid = uint64_t(64) * c->ncu;
    if (!c->serial_walk) {
        // parallel walk: sync search, part walks, per-segment fix-up, record
        // emission; the serial walker then takes only the segments the fix-up
        // handed back (uint32_t wraps, exhausted re-walk budget)
        // part size: chosen per batch on the device by k_walk_probe from the
        // entry density (or forced, RAMCRC_OPT_WALK_PART_SHIFT); grids and
        // scratch are sized for the smallest part it may choose
        const uint32_t pshift = c->walk_pshift ? c->walk_pshift : kPartShiftLow;
        const uint32_t nparts = uint32_t((uint64_t(seg_capacity) + (1ull << pshift) - 1) >> pshift);
        const uint64_t total = n_seg * uint64_t(nparts);
        int rc = grow_device(&c->walk_parts, &c->walk_parts_cap, total, sizeof(PartRes));
        if (!rc)
            rc = grow_device(reinterpret_cast<void**>(&c->walk_fallback), &c->walk_fallback_cap,
                             n_seg, sizeof(uint32_t));
        if (!rc)
            rc = grow_device(&c->walk_recs, &c->walk_recs_cap, total * kPartRec, sizeof(uint2));
        // the pool holds A's records past each part's first block: sized for
        // entries of 96 B on average (denser parts than that, and records past
        // entries_cap, fall back to C's second walk of the part)
        uint64_t pool_blocks = (n_seg * uint64_t(seg_capacity) / 96) / kPartRec + 1;
        const uint64_t cap_blocks = entries_cap / kPartRec + 1;
        pool_blocks = pool_blocks < cap_blocks ? pool_blocks : cap_blocks;
        if (!rc)
            rc = grow_device(&c->walk_pool, &c->walk_pool_cap, pool_blocks * kPartRec, sizeof(uint2));
        if (!rc)
            rc = grow_device(reinterpret_cast<void**>(&c->walk_pool_owner), &c->walk_pool_owner_cap,
                             pool_blocks, sizeof(uint32_t));
        if (!rc)
            rc = grow_device(reinterpret_cast<void**>(&c->walk_blocks), &c->walk_blocks_cap,
                             total * kMaxBlocks, sizeof(uint32_t));
        if (!rc)
            rc = grow_device(reinterpret_cast<void**>(&c->walk_pool_used), &c->walk_pool_used_cap, 3,
                             sizeof(unsigned long long));   // [1]: the part shift word, [2]: k_left's count
        // verify-in-walk mode (fused call): the list of records k_left checks
        const uint64_t left_cap = entries_cap / 8 + 65536 < entries_cap ? entries_cap / 8 + 65536 : entries_cap;
        if (!rc && d_obj_crc && sum)
            rc = grow_device(reinterpret_cast<void**>(&c->walk_left), &c->walk_left_cap, left_cap,
                             sizeof(uint32_t));
        if (rc)
            return rc;
        PWalk pw{};
        pw.base = w.base;
        pw.stride = seg_stride;
        pw.capacity = seg_capacity;
        pw.nparts = nparts;
        pw.nseg = n_seg;
        pw.certs = d_certs;
        pw.status = d_status;
        pw.entries = w.entries;
        pw.cap = entries_cap;
        pw.n_entries = w.n_entries;
        pw.parts = static_cast<PartRes*>(c->walk_parts);
        pw.fallback = c->walk_fallback;
        pw.seg_base = c->walk_base;
        pw.recs = static_cast<uint2*>(c->walk_recs);
        pw.pshift = pshift;
        uint32_t* geo = reinterpret_cast<uint32_t*>(c->walk_pool_used + 1);
        pw.geo = geo;
        pw.pool = static_cast<uint2*>(c->walk_pool);
        pw.pool_owner = c->walk_pool_owner;
        pw.blocks = c->walk_blocks;
        pw.pool_used = c->walk_pool_used;
        pw.pool_cap = pool_blocks;
        pw.sum = sum;
        if (d_obj_crc && sum) {
            pw.obj_crc = d_obj_crc;
            pw.left = c->walk_left;
            pw.nleft = c->walk_pool_used + 2;
            pw.left_cap = left_cap;
            pw.vmode = uint32_t(c->verify_in_walk);
        }
        // The pool block map starts empty on every call: the part -> block
        // table (blocks) and the block -> part table (pool_owner) of the
        // previous call on this context are stale, and the fix-up's block
        // replacement reads them.  Carried over, they gave wrong records on a
        // repeated call when the fix-up re-walked parts with pool blocks
        // (replay of 2 and 3 KiB values, 256 KiB parts: records of one part's
        // pool block replaced by another's, found in round 6 by the bench's
        // object-CRC check, tests/test_gpu_replay_fused.py::
        // test_repeated_calls_pool_blocks).
        HIPCHK(hipMemsetAsync(c->walk_blocks, 0xFF, total * kMaxBlocks * sizeof(uint32_t), s));
        HIPCHK(hipMemsetAsync(c->walk_pool_owner, 0xFF, pool_blocks * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_walk_probe, dim3(1), dim3(kWaveSize), 0, s, pw, c->walk_pshift, geo);
        HIPCHK(hipGetLastError());
        if (nparts > 1) {
            uint64_t g0 = (total + kSyncWaves - 1) / kSyncWaves;
            if (g0 > uint64_t(8) * c->ncu)
                g0 = uint64_t(8) * c->ncu;
            hipLaunchKernelGGL(k_walk_sync, dim3(g0), dim3(kSyncWaves * kWaveSize), 0, s, pw);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_walk_parts, dim3((total + 255) / 256), dim3(256), 0, s, pw);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_walk_fix, dim3(grid), dim3(kWaveSize), 0, s, pw);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_walk_emit, dim3((total + 255) / 256), dim3(256), 0, s, pw);
        HIPCHK(hipGetLastError());
        uint64_t gc = (total + pool_blocks + 4 * kCopyU - 1) / (4 * kCopyU);   // kCopyU blocks per wave
        if (gc > uint64_t(32) * c->ncu)
            gc = uint64_t(32) * c->ncu;
        hipLaunchKernelGGL(k_walk_copy, dim3(gc), dim3(256), 0, s, pw);
        HIPCHK(hipGetLastError());
        if (pw.obj_crc) {   // verify-in-walk mode, decided by k_walk_probe (else it exits)
            uint64_t gv = (total + kVWaves - 1) / kVWaves;   // a wave per part
            if (gv > uint64_t(16) * c->ncu)
                gv = uint64_t(16) * c->ncu;
            // (the probe picks the stage size; the other instantiation exits).
            // Timed with the scan kernels: in this mode they do the object
            // checks k_entries does otherwise.
            {
                ScanTimer t(c, s);
                t.launch(k_walk_copyv<kVStageS>, dim3(gv), dim3(kVWaves * kWaveSize), pw);
            }
            HIPCHK(hipGetLastError());
            {
                ScanTimer t(c, s);
                t.launch(k_walk_copyv<kVStageL>, dim3(gv), dim3(kVWaves * kWaveSize), pw);
            }
            HIPCHK(hipGetLastError());
        }
        w.only = c->walk_fallback;
    }
    hipLaunchKernelGGL(k_seg_walk, dim3(grid), dim3(kWaveSize), 0, s, w);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}
}  // namespace

int ramcrc_segments_certify_device(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride,
                                   uint32_t seg_capacity, uint64_t n_seg, const uint32_t* d_heads,
                                   ramcrc_seg_cert* d_certs, uint32_t* d_flags, void* stream)
{
    if (!c)
        return RAMCRC_EINVAL;
    if (n_seg == 0)
        return RAMCRC_OK;
    if (!d_base || !d_heads || !d_certs || n_seg > 0xFFFFFFFFull)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch: placeholder certificates, walk status, the walk's entry count
    const uint64_t need = n_seg * (sizeof(ramcrc_seg_cert) + sizeof(ramcrc_seg_status)) / 4 + 2;
    int rc = grow_device(reinterpret_cast<void**>(&c->cert_scratch), &c->cert_scratch_cap, need,
                         sizeof(uint32_t));
    if (rc)
        return rc;
    uint64_t* d_n = reinterpret_cast<uint64_t*>(c->cert_scratch);
    ramcrc_seg_cert* tmp = reinterpret_cast<ramcrc_seg_cert*>(c->cert_scratch + 2);
    ramcrc_seg_status* st = reinterpret_cast<ramcrc_seg_status*>(tmp + n_seg);
    const dim3 grid(uint32_t((n_seg + 255) / 256));
    hipLaunchKernelGGL(k_cert_prep, grid, dim3(256), 0, s, d_heads, tmp, n_seg);
    HIPCHK(hipGetLastError());
    rc = ramcrc_segment_walk_device(c, d_base, seg_stride, seg_capacity, n_seg, tmp, st, nullptr, 0,
                                    d_n, stream);
    if (rc)
        return rc;
    hipLaunchKernelGGL(k_cert_emit, grid, dim3(256), 0, s, tmp, st, d_certs, d_flags, n_seg);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

namespace {
// The append's checks and launches, shared by ramcrc_recovery_append_device
// (sl == nullptr: exactly k_app_mark, k_app_scan, k_app_copy) and
// ramcrc_replay_sidelog_device (k_sl_stamp behind them; sl->counts is set
// here, to a line of its own behind the append's scratch words).
int app_launch(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride, uint64_t n_seg,
               const ramcrc_seg_status* d_status, const ramcrc_seg_entry* d_entries,
               uint64_t entries_cap, const uint64_t* d_n_entries, const ramcrc_placement* d_place,
               uint64_t place_cap, const uint64_t* d_n_place, uint32_t n_part, void* d_out,
               uint64_t out_stride, uint32_t out_capacity, ramcrc_seg_cert* d_out_certs,
               ramcrc_append_status* d_out_status, SlDesc* sl, void* stream)
{
    if (!c || n_part == 0 || out_stride < out_capacity || n_seg > 0xFFFFFFFFull ||
        place_cap > 0xFFFFFFFFull)
        return RAMCRC_EINVAL;
    if (n_seg == 0)
        return RAMCRC_OK;
    if (!d_base || !d_status || !d_n_entries || !d_n_place || !d_out || !d_out_certs ||
        !d_out_status || (entries_cap && !d_entries) || (place_cap && !d_place))
        return RAMCRC_EINVAL;
    const uint64_t B = reinterpret_cast<uint64_t>(d_base), O = reinterpret_cast<uint64_t>(d_out);
    if ((B & 15) || (seg_stride & 15))
        return RAMCRC_EINVAL;
    const uint64_t n_out = n_seg * n_part;   // both below 2^32
    if ((seg_stride && n_seg > UINT64_MAX / seg_stride) ||
        (out_stride && n_out > UINT64_MAX / out_stride) || n_out > UINT64_MAX / sizeof(AppState))
        return RAMCRC_EINVAL;
    const uint64_t src_bytes = n_seg * seg_stride, out_bytes = n_out * out_stride;
    if (B > UINT64_MAX - src_bytes || O > UINT64_MAX - out_bytes ||
        (B < O + out_bytes && O < B + src_bytes))
        return RAMCRC_EINVAL;   // the outputs would overwrite the source
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch words in the chunk-partial buffer: the refusal word, the
    // segments' runs, then the scan states when they do not fit in LDS; the
    // placements' offsets in the plan buffer (ramcrc.h states these sizes)
    const uint64_t head_words = (4 + 3 * n_seg + 3) & ~uint64_t(3);
    const uint64_t state_words = n_part > kAppLdsParts ? n_out * (sizeof(AppState) / 4) : 0;
    const uint64_t app_words = head_words + state_words;
    const uint64_t sl_at = (app_words + kSlCountWords - 1) / kSlCountWords * kSlCountWords;
    int rc = reserve_locked(c, sl ? sl_at + kSlCountWords : app_words, place_cap / 2 + 1);
    if (rc)
        return rc;
    AppDesc a{};
    a.base = B;
    a.stride = seg_stride;
    a.nseg = n_seg;
    a.status = d_status;
    a.entries = reinterpret_cast<const u32x4*>(d_entries);
    a.ecap = entries_cap;
    a.n_entries = d_n_entries;
    a.place = reinterpret_cast<const uint2*>(d_place);
    a.pcap = place_cap;
    a.n_place = d_n_place;
    a.npart = n_part;
    a.ocap = out_capacity;
    a.out = O;
    a.ostride = out_stride;
    a.certs = d_out_certs;
    a.ostat = d_out_status;
    a.refuse = c->partials;
    a.run_lo = c->partials + 4;
    a.run_hi = a.run_lo + n_seg;
    a.run_cnt = a.run_hi + n_seg;
    a.pdst = reinterpret_cast<uint32_t*>(c->plan_local);
    a.states = reinterpret_cast<AppState*>(c->partials + head_words);
    a.ctx_status = c->status;
    HIPCHK(hipMemsetAsync(c->partials, 0, head_words * sizeof(uint32_t), s));
    if (sl) {
        sl->counts = reinterpret_cast<unsigned long long*>(c->partials + sl_at);
        HIPCHK(hipMemsetAsync(sl->counts, 0, kSlCountWords * sizeof(uint32_t), s));
    }
    const uint64_t cap_grid = uint64_t(8) * c->ncu;
    uint64_t gm = (place_cap + 255) / 256;
    gm = gm < 1 ? 1 : (gm > cap_grid ? cap_grid : gm);
    hipLaunchKernelGGL(k_app_mark, dim3(uint32_t(gm)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    // waves per source segment: about 16 waves per CU in all, at most 8 and
    // no more than there are partitions
    uint32_t nown = 1;
    while (nown < 8 && 2 * nown <= n_part && n_seg * (2 * nown) <= uint64_t(16) * c->ncu)
        nown *= 2;
    a.nown = nown;
    const uint64_t gs = n_seg * nown < uint64_t(16) * c->ncu ? n_seg * nown : uint64_t(16) * c->ncu;
    if (n_part <= kAppLdsParts)
        hipLaunchKernelGGL(k_app_scan<true>, dim3(uint32_t(gs)), dim3(kWaveSize), 0, s, a);
    else
        hipLaunchKernelGGL(k_app_scan<false>, dim3(uint32_t(gs)), dim3(kWaveSize), 0, s, a);
    HIPCHK(hipGetLastError());
    if (place_cap) {
        uint64_t gc = (place_cap + kAppCopyThreads - 1) / kAppCopyThreads;
        gc = gc > cap_grid ? cap_grid : gc;
        hipLaunchKernelGGL(k_app_copy, dim3(uint32_t(gc)), dim3(kAppCopyThreads), 0, s, a);
        HIPCHK(hipGetLastError());
    }
    if (sl) {
        // (at least one workgroup: an empty list still gets its zero counts)
        uint64_t gt = (place_cap + kSlThreads - 1) / kSlThreads;
        gt = gt < 1 ? 1 : (gt > cap_grid ? cap_grid : gt);
        hipLaunchKernelGGL(k_sl_stamp, dim3(uint32_t(gt)), dim3(kSlThreads), 0, s, a, *sl);
        HIPCHK(hipGetLastError());
    }
    return RAMCRC_OK;
}
}  // namespace

int ramcrc_recovery_append_device(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride,
                                  uint64_t n_seg, const ramcrc_seg_status* d_status,
                                  const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                  const uint64_t* d_n_entries, const ramcrc_placement* d_place,
                                  uint64_t place_cap, const uint64_t* d_n_place, uint32_t n_part,
                                  void* d_out, uint64_t out_stride, uint32_t out_capacity,
                                  ramcrc_seg_cert* d_out_certs, ramcrc_append_status* d_out_status,
                                  void* stream)
{
    return app_launch(c, d_base, seg_stride, n_seg, d_status, d_entries, entries_cap, d_n_entries,
                      d_place, place_cap, d_n_place, n_part, d_out, out_stride, out_capacity,
                      d_out_certs, d_out_status, nullptr, stream);
}

int ramcrc_replay_sidelog_device(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride,
                                 uint64_t n_seg, const ramcrc_seg_status* d_status,
                                 const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                 const uint64_t* d_n_entries, const ramcrc_placement* d_live,
                                 uint64_t live_cap, const uint64_t* d_n_live, uint32_t timestamp,
                                 void* d_out, uint64_t out_stride, uint32_t out_capacity,
                                 ramcrc_seg_cert* d_out_certs, ramcrc_append_status* d_out_status,
                                 ramcrc_log_ref* d_refs, ramcrc_sidelog_counts* d_counts,
                                 void* stream)
{
    if (!d_counts)
        return RAMCRC_EINVAL;
    SlDesc sl{};
    sl.refs = reinterpret_cast<uint2*>(d_refs);
    sl.counts_out = d_counts;
    sl.timestamp = timestamp;
    return app_launch(c, d_base, seg_stride, n_seg, d_status, d_entries, entries_cap, d_n_entries,
                      d_live, live_cap, d_n_live, 1, d_out, out_stride, out_capacity, d_out_certs,
                      d_out_status, &sl, stream);
}

int ramcrc_recovery_partition_device(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride,
                                     uint64_t n_seg, const ramcrc_seg_status* d_status,
                                     const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                     const uint64_t* d_n_entries, const ramcrc_tablet* d_tablets,
                                     uint32_t n_tablets, uint32_t n_part,
                                     ramcrc_placement* d_place, uint64_t place_cap,
                                     uint64_t* d_n_place, uint64_t* d_key_hash,
                                     ramcrc_partition_status* d_part_status, void* stream)
{
    if (!c || n_seg >= 0xFFFFFFFFull || entries_cap >= 0xFFFFFFFFull || place_cap >= 0xFFFFFFFFull)
        return RAMCRC_EINVAL;
    if (!d_n_place || !d_n_entries || (n_seg && (!d_base || !d_status || !d_part_status)) ||
        (entries_cap && !d_entries) || (place_cap && !d_place) || (n_tablets && !d_tablets))
        return RAMCRC_EINVAL;
    const uint64_t B = reinterpret_cast<uint64_t>(d_base);
    if ((B & 15) || (seg_stride & 15) || (seg_stride && n_seg > UINT64_MAX / seg_stride))
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch words in the chunk-partial buffer: the refusal word, then nine
    // words per segment (runs, headers, flags, counters); the records' counts
    // in the plan buffer and the tile sums in the group prefixes (ramcrc.h
    // states these sizes)
    const uint64_t head_words = 4 + 9 * n_seg;
    int rc = reserve_locked(c, head_words, entries_cap);
    if (rc)
        return rc;
    PartDesc a{};
    a.base = B;
    a.stride = seg_stride;
    a.nseg = n_seg;
    a.status = d_status;
    a.entries = reinterpret_cast<const u32x4*>(d_entries);
    a.ecap = entries_cap;
    a.n_entries = d_n_entries;
    a.tablets = d_tablets;
    a.ntab = n_tablets;
    a.npart = n_part;
    a.place = reinterpret_cast<uint2*>(d_place);
    a.pcap = place_cap;
    a.n_place = d_n_place;
    a.key_hash = d_key_hash;
    a.pstat = d_part_status;
    a.refuse = c->partials;
    a.run_lo = c->partials + 4;
    a.run_hi = a.run_lo + n_seg;
    a.run_cnt = a.run_hi + n_seg;
    a.hdr_cnt = a.run_cnt + n_seg;
    a.hdr_first = a.hdr_cnt + n_seg;
    a.sflags = a.hdr_first + n_seg;
    a.counts = a.sflags + n_seg;
    a.cls = c->plan_local;
    a.tile_sum = c->group_pref;
    a.ctx_status = c->status;
    HIPCHK(hipMemsetAsync(c->partials, 0, head_words * sizeof(uint32_t), s));
    const uint64_t cap_grid = uint64_t(8) * c->ncu;
    auto grid_of = [&](uint64_t items, uint64_t per) {
        uint64_t gr = (items + per - 1) / per;
        return dim3(uint32_t(gr < 1 ? 1 : (gr > cap_grid ? cap_grid : gr)));
    };
    const uint64_t heads_items = entries_cap > n_tablets ? entries_cap : n_tablets;
    hipLaunchKernelGGL(k_part_heads, grid_of(heads_items, kPartThreads), dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    if (n_tablets <= kPartLdsTablets)
        hipLaunchKernelGGL(k_part_classify<true>, grid_of(entries_cap, kPartThreads),
                           dim3(kPartThreads), 0, s, a);
    else
        hipLaunchKernelGGL(k_part_classify<false>, grid_of(entries_cap, kPartThreads),
                           dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_part_void, grid_of(n_seg, 1), dim3(kWaveSize), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_part_tiles, grid_of(entries_cap, kPartTile), dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_part_scan, dim3(1), dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_part_emit, grid_of(entries_cap, kPartTile), dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

int ramcrc_replay_resolve_device(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride,
                                 uint64_t n_seg, const ramcrc_seg_status* d_status,
                                 const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                 const uint64_t* d_n_entries, const uint64_t* d_key_hash,
                                 uint32_t* d_winner, ramcrc_placement* d_live, uint64_t live_cap,
                                 uint64_t* d_n_live, ramcrc_resolve_counts* d_counts, void* stream)
{
    if (!c || n_seg >= 0xFFFFFFFFull || entries_cap >= 0xFFFFFFFFull || live_cap >= 0xFFFFFFFFull)
        return RAMCRC_EINVAL;
    if (!d_n_live || !d_counts || !d_n_entries || (n_seg && (!d_base || !d_status)) ||
        (entries_cap && !d_entries) || (live_cap && !d_live))
        return RAMCRC_EINVAL;
    const uint64_t B = reinterpret_cast<uint64_t>(d_base);
    if ((B & 15) || (seg_stride & 15) || (seg_stride && n_seg > UINT64_MAX / seg_stride))
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch words in the chunk-partial buffer: the head (refusal word and
    // counters), then six words per slot of the largest grouping table this
    // shape can need; a version and a slot per record in the plan buffer and
    // the tile sums in the group prefixes (ramcrc.h states these sizes)
    const uint64_t slots = ramcrc_res::slots_for(entries_cap);
    int rc = reserve_locked(c, kResHeadWords + 2 * kResSlotWords * slots, 2 * entries_cap);
    if (rc)
        return rc;
    ResDesc a{};
    a.base = B;
    a.stride = seg_stride;
    a.nseg = n_seg;
    a.status = d_status;
    a.entries = reinterpret_cast<const u32x4*>(d_entries);
    a.ecap = entries_cap;
    a.n_entries = d_n_entries;
    a.key_hash = d_key_hash;
    a.winner = d_winner;
    a.live = reinterpret_cast<uint2*>(d_live);
    a.lcap = live_cap;
    a.n_live = d_n_live;
    a.counts_out = d_counts;
    a.refuse = c->partials;
    a.counts = reinterpret_cast<unsigned long long*>(c->partials + 4);
    a.slots = reinterpret_cast<unsigned long long*>(c->partials + kResHeadWords);
    a.rec_ver = c->plan_local;
    a.rec_slot = c->plan_local + entries_cap;
    a.tile_sum = c->group_pref;
    a.ctx_status = c->status;
    HIPCHK(hipMemsetAsync(c->partials, 0, kResHeadWords * sizeof(uint32_t), s));
    const uint64_t cap_grid = uint64_t(8) * c->ncu;
    auto grid_of = [&](uint64_t items, uint64_t per) {
        uint64_t gr = (items + per - 1) / per;
        return dim3(uint32_t(gr < 1 ? 1 : (gr > cap_grid ? cap_grid : gr)));
    };
    hipLaunchKernelGGL(k_res_zero, grid_of(kResSlotWords * slots, kPartThreads), dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    if (d_key_hash)
        hipLaunchKernelGGL(k_res_insert<true>, grid_of(entries_cap, kPartThreads), dim3(kPartThreads),
                           0, s, a);
    else
        hipLaunchKernelGGL(k_res_insert<false>, grid_of(entries_cap, kPartThreads), dim3(kPartThreads),
                           0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_res_pick, grid_of(entries_cap, kPartThreads), dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_res_tiles, grid_of(entries_cap, kPartTile), dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_res_scan, dim3(1), dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_res_emit, grid_of(entries_cap, kPartTile), dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

struct ramcrc_replay_table {
    ramcrc_ctx* ctx = nullptr;
    std::mutex mu;              // serialises the calls on this table
    unsigned long long* mem = nullptr;   // the head, the descriptors, the batches' counters, the slots
    uint64_t key_cap = 0, nslots = 0;
    uint32_t max_batches = 0;
    std::vector<uint64_t> ecap;   // entries_cap of every batch numbered since the last reset
    std::vector<uint8_t> retired; // 1: the batch was cleaned out (ramcrc_replay_table_clean_device)
};

namespace {
RtabDesc rtab_desc(const ramcrc_replay_table* t)
{
    RtabDesc a{};
    a.head = t->mem;
    a.batches = reinterpret_cast<RtabBatch*>(t->mem + kRtabHeadWords);
    a.bcount = reinterpret_cast<RtabCount*>(a.batches + t->max_batches);
    a.slots = reinterpret_cast<unsigned long long*>(a.bcount + t->max_batches);
    a.nslots = t->nslots;
    a.key_cap = t->key_cap;
    a.n_batches = uint32_t(t->ecap.size());
    a.ctx_status = t->ctx->status;
    return a;
}

// Workgroups for `items` at `per` a workgroup: at most 8 per CU, at least one.
uint32_t rtab_grid(const ramcrc_ctx* c, uint64_t items, uint64_t per)
{
    const uint64_t cap_grid = uint64_t(8) * c->ncu;
    const uint64_t gr = (items + per - 1) / per;
    return uint32_t(gr < 1 ? 1 : (gr > cap_grid ? cap_grid : gr));
}
}  // namespace

int ramcrc_replay_table_create(ramcrc_ctx* c, uint64_t key_cap, uint32_t max_batches,
                               ramcrc_replay_table** out)
{
    if (!out)
        return RAMCRC_EINVAL;
    *out = nullptr;
    if (!c || key_cap >= 0xFFFFFFFFull || max_batches == 0 || max_batches > RAMCRC_REPLAY_TABLE_MAX_BATCHES)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    ramcrc_replay_table* t = new (std::nothrow) ramcrc_replay_table();
    if (!t)
        return RAMCRC_ENOMEM;
    t->ctx = c;
    t->key_cap = key_cap;
    t->nslots = ramcrc_res::slots_for(key_cap);
    t->max_batches = max_batches;
    const uint64_t words =
        kRtabHeadWords + ((sizeof(RtabBatch) + sizeof(RtabCount)) / 8) * max_batches +
        kRtabSlotWords * t->nslots;
    if (hipMalloc(reinterpret_cast<void**>(&t->mem), words * 8) != hipSuccess) {
        delete t;
        return RAMCRC_ENOMEM;
    }
    if (hipMemset(t->mem, 0, words * 8) != hipSuccess) {
        (void)hipFree(t->mem);
        delete t;
        return RAMCRC_EHIP;
    }
    *out = t;
    return RAMCRC_OK;
}

int ramcrc_replay_table_destroy(ramcrc_replay_table* t)
{
    if (!t)
        return RAMCRC_OK;
    {
        DeviceGuard g(t->ctx->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(t->mem);
    }
    delete t;
    return RAMCRC_OK;
}

int ramcrc_replay_table_reset(ramcrc_replay_table* t, void* stream)
{
    if (!t)
        return RAMCRC_EINVAL;
    std::lock_guard<std::mutex> lt(t->mu);
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    const RtabDesc a = rtab_desc(t);
    hipLaunchKernelGGL(k_rtab_zero, dim3(rtab_grid(c, kRtabSlotWords * t->nslots, kPartThreads)),
                       dim3(kPartThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
    HIPCHK(hipGetLastError());
    t->ecap.clear();
    t->retired.clear();
    return RAMCRC_OK;
}

int ramcrc_replay_table_add_device(ramcrc_replay_table* t, const void* d_base, uint64_t seg_stride,
                                   uint64_t n_seg, const ramcrc_seg_status* d_status,
                                   const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                   const uint64_t* d_n_entries, const uint64_t* d_key_hash,
                                   uint64_t* d_work, uint32_t* batch, void* stream)
{
    if (!t || n_seg >= 0xFFFFFFFFull || entries_cap >= 0xFFFFFFFFull)
        return RAMCRC_EINVAL;
    if (!d_n_entries || (n_seg && (!d_base || !d_status)) ||
        (entries_cap && (!d_entries || !d_work)))
        return RAMCRC_EINVAL;
    const uint64_t B = reinterpret_cast<uint64_t>(d_base);
    if ((B & 15) || (seg_stride & 15) || (seg_stride && n_seg > UINT64_MAX / seg_stride))
        return RAMCRC_EINVAL;
    std::lock_guard<std::mutex> lt(t->mu);
    if (t->ecap.size() >= t->max_batches)
        return RAMCRC_EINVAL;
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    RtabDesc a = rtab_desc(t);
    a.batch = uint32_t(t->ecap.size());
    a.open.base = B;
    a.open.stride = seg_stride;
    a.open.nseg = n_seg;
    a.open.status = d_status;
    a.open.entries = reinterpret_cast<const u32x4*>(d_entries);
    a.open.n_entries = d_n_entries;
    a.open.ecap = entries_cap;
    a.open.key_hash = d_key_hash;
    a.open.work = d_work;
    // the descriptor travels in the kernel's arguments: the add stays
    // capturable and no host memory has to outlive the call
    hipLaunchKernelGGL(k_rtab_open, dim3(1), dim3(kWaveSize), 0, s, a);
    HIPCHK(hipGetLastError());
    t->ecap.push_back(entries_cap);
    t->retired.push_back(0);
    if (batch)
        *batch = a.batch;
    const dim3 grid(rtab_grid(c, entries_cap, kPartThreads));
    if (d_key_hash)
        hipLaunchKernelGGL(k_rtab_insert<true>, grid, dim3(kPartThreads), 0, s, a);
    else
        hipLaunchKernelGGL(k_rtab_insert<false>, grid, dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rtab_pick, grid, dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

int ramcrc_replay_table_live_device(ramcrc_replay_table* t, uint32_t batch,
                                    ramcrc_replay_ref* d_winner, ramcrc_placement* d_live,
                                    uint64_t live_cap, uint64_t* d_n_live,
                                    ramcrc_resolve_counts* d_counts, void* stream)
{
    if (!t || !d_n_live || !d_counts || live_cap >= 0xFFFFFFFFull || (live_cap && !d_live))
        return RAMCRC_EINVAL;
    std::lock_guard<std::mutex> lt(t->mu);
    if (batch >= t->ecap.size() || t->retired[batch])
        return RAMCRC_EINVAL;
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint64_t ecap = t->ecap[batch];
    // the tile sums: the group prefixes, sized as ramcrc_ctx_reserve sizes them
    int rc = grow_device(reinterpret_cast<void**>(&c->group_pref), &c->group_cap,
                         (ecap + kThreads - 1) / kThreads + 1, sizeof(uint64_t));
    if (rc)
        return rc;
    RtabDesc a = rtab_desc(t);
    a.batch = batch;
    a.winner = reinterpret_cast<uint2*>(d_winner);
    a.live = reinterpret_cast<uint2*>(d_live);
    a.lcap = live_cap;
    a.n_live = d_n_live;
    a.counts_out = d_counts;
    a.tile_sum = c->group_pref;
    const dim3 grid(rtab_grid(c, ecap, kPartTile));
    hipLaunchKernelGGL(k_rtab_tiles, grid, dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rtab_scan, dim3(1), dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rtab_emit, grid, dim3(kPartThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

int ramcrc_replay_table_stats_device(ramcrc_replay_table* t, ramcrc_replay_table_stats* d_stats,
                                     void* stream)
{
    if (!t || !d_stats)
        return RAMCRC_EINVAL;
    std::lock_guard<std::mutex> lt(t->mu);
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    RtabDesc a = rtab_desc(t);
    a.stats_out = d_stats;
    HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(*d_stats), s));
    hipLaunchKernelGGL(k_rtab_stats, dim3(rtab_grid(c, t->nslots, kPartThreads)), dim3(kPartThreads),
                       0, s, a);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

int ramcrc_replay_table_lookup_device(ramcrc_replay_table* t, const void* d_keys, uint64_t keys_bytes,
                                      const ramcrc_lookup_key* d_queries, uint64_t n_queries,
                                      const uint64_t* d_key_hash, ramcrc_lookup_result* d_results,
                                      ramcrc_lookup_counts* d_counts, void* stream)
{
    if (!t || n_queries >= 0xFFFFFFFFull || (n_queries && (!d_queries || !d_results)) ||
        (keys_bytes && !d_keys))
        return RAMCRC_EINVAL;
    const uint64_t K = reinterpret_cast<uint64_t>(d_keys);
    if ((reinterpret_cast<uint64_t>(d_queries) & 7) || (reinterpret_cast<uint64_t>(d_results) & 15) ||
        K > UINT64_MAX - keys_bytes)
        return RAMCRC_EINVAL;
    if (n_queries == 0 && !d_counts)
        return RAMCRC_OK;
    std::lock_guard<std::mutex> lt(t->mu);
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // the counters: the first line of the chunk-partial buffer (ramcrc.h
    // states this size)
    int rc = reserve_locked(c, kLookCountWords, 0);
    if (rc)
        return rc;
    const RtabDesc a = rtab_desc(t);
    LookDesc q{};
    q.keys = K;
    q.keys_bytes = keys_bytes;
    q.queries = reinterpret_cast<const uint64_t*>(d_queries);
    q.nq = n_queries;
    q.key_hash = d_key_hash;
    q.results = reinterpret_cast<u32x4*>(d_results);
    q.counts_out = d_counts;
    q.counts = reinterpret_cast<unsigned long long*>(c->partials);
    if (d_counts)
        HIPCHK(hipMemsetAsync(q.counts, 0, kLookCountWords * sizeof(uint32_t), s));
    // (at least one workgroup: an empty call still gets its counts)
    const dim3 grid(rtab_grid(c, n_queries, kPartThreads));
    if (d_key_hash)
        hipLaunchKernelGGL(k_rtab_lookup<true>, grid, dim3(kPartThreads), 0, s, a, q);
    else
        hipLaunchKernelGGL(k_rtab_lookup<false>, grid, dim3(kPartThreads), 0, s, a, q);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

int ramcrc_replay_table_read_device(ramcrc_replay_table* t, const void* d_keys, uint64_t keys_bytes,
                                    const ramcrc_lookup_key* d_queries, uint64_t n_queries,
                                    const uint64_t* d_key_hash, const ramcrc_reject_rules* d_rules,
                                    uint32_t flags, void* d_reply, uint64_t reply_cap,
                                    uint64_t* d_part_off, ramcrc_lookup_result* d_results,
                                    ramcrc_read_summary* d_summary, void* stream)
{
    if (!t || n_queries >= 0xFFFFFFFFull || (flags & ~RAMCRC_READ_VALUE_ONLY) ||
        (n_queries && (!d_queries || !d_summary)) || (keys_bytes && !d_keys) ||
        (reply_cap && !d_reply))
        return RAMCRC_EINVAL;
    const uint64_t K = reinterpret_cast<uint64_t>(d_keys), R = reinterpret_cast<uint64_t>(d_reply);
    if ((reinterpret_cast<uint64_t>(d_queries) & 7) || (reinterpret_cast<uint64_t>(d_rules) & 7) ||
        (reinterpret_cast<uint64_t>(d_results) & 15) || (reinterpret_cast<uint64_t>(d_part_off) & 7) ||
        (reinterpret_cast<uint64_t>(d_summary) & 7) || K > UINT64_MAX - keys_bytes ||
        R > UINT64_MAX - reply_cap)
        return RAMCRC_EINVAL;
    if (!d_summary)
        return RAMCRC_OK;
    std::lock_guard<std::mutex> lt(t->mu);
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch: a line for the scan's word to the gather, then the tile sums,
    // in the chunk-partial buffer; the per-query words in the plan buffer
    // (ramcrc.h states these sizes)
    const uint64_t ntiles = (n_queries + kPartThreads - 1) / kPartThreads;
    int rc = reserve_locked(c, kLookCountWords + 2 * kReadTileWords * ntiles, kReadRecWords * n_queries);
    if (rc)
        return rc;
    const RtabDesc a = rtab_desc(t);
    LookDesc q{};
    q.keys = K;
    q.keys_bytes = keys_bytes;
    q.queries = reinterpret_cast<const uint64_t*>(d_queries);
    q.nq = n_queries;
    q.key_hash = d_key_hash;
    q.results = reinterpret_cast<u32x4*>(d_results);
    ReadDesc r{};
    r.rules = reinterpret_cast<const uint64_t*>(d_rules);
    r.flags = flags;
    r.reply = R;
    r.cap = reply_cap;
    r.part_off = d_part_off;
    r.summary = d_summary;
    r.rec = c->plan_local;
    r.head = reinterpret_cast<unsigned long long*>(c->partials);
    r.tile = reinterpret_cast<uint64_t*>(c->partials + kLookCountWords);
    const dim3 grid(rtab_grid(c, n_queries, kPartThreads));
    if (n_queries) {
        HIPCHK(hipMemsetAsync(r.tile, 0, kReadTileWords * ntiles * sizeof(uint64_t), s));
        if (d_key_hash)
            hipLaunchKernelGGL(k_rtab_read_size<true>, grid, dim3(kPartThreads), 0, s, a, q, r);
        else
            hipLaunchKernelGGL(k_rtab_read_size<false>, grid, dim3(kPartThreads), 0, s, a, q, r);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_rtab_read_scan, dim3(1), dim3(kPartThreads), 0, s, a, q, r);
    HIPCHK(hipGetLastError());
    if (n_queries) {
        hipLaunchKernelGGL(k_rtab_read_gather, grid, dim3(kPartThreads), 0, s, a, q, r);
        HIPCHK(hipGetLastError());
    }
    return RAMCRC_OK;
}

int ramcrc_replay_table_read_hashes_device(ramcrc_replay_table* t, uint64_t table_id,
                                           const uint64_t* d_hashes, uint64_t n_hashes, uint32_t flags,
                                           void* d_reply, uint64_t reply_capacity, uint64_t max_length,
                                           ramcrc_hash_part* d_parts, ramcrc_read_hashes_summary* d_summary,
                                           void* stream)
{
    if (!t || flags != 0 || !d_summary || n_hashes >= 0xFFFFFFFFull || (n_hashes && !d_hashes) ||
        (reply_capacity && !d_reply))
        return RAMCRC_EINVAL;
    const uint64_t R = reinterpret_cast<uint64_t>(d_reply);
    if ((reinterpret_cast<uint64_t>(d_hashes) & 7) || (reinterpret_cast<uint64_t>(d_parts) & 7) ||
        (reinterpret_cast<uint64_t>(d_summary) & 7) || R > UINT64_MAX - reply_capacity)
        return RAMCRC_EINVAL;
    std::lock_guard<std::mutex> lt(t->mu);
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch: a line for the scan's word to the gather, then the tile sums,
    // in the chunk-partial buffer; the per-hash words in the plan buffer
    // (ramcrc.h states these sizes)
    const uint64_t ntiles = (n_hashes + kPartThreads - 1) / kPartThreads;
    int rc = reserve_locked(c, kLookCountWords + 2 * kRhTileStride * ntiles, kRhRecWords * n_hashes);
    if (rc)
        return rc;
    const RtabDesc a = rtab_desc(t);
    RhDesc r{};
    r.table_id = table_id;
    r.hashes = d_hashes;
    r.nq = n_hashes;
    r.reply = R;
    r.cap = reply_capacity;
    r.max_length = max_length;
    r.parts = reinterpret_cast<uint64_t*>(d_parts);
    r.summary = d_summary;
    r.rec = c->plan_local;
    r.head = reinterpret_cast<unsigned long long*>(c->partials);
    r.tile = reinterpret_cast<uint64_t*>(c->partials + kLookCountWords);
    const dim3 grid(rtab_grid(c, n_hashes, kPartThreads));
    if (n_hashes) {
        HIPCHK(hipMemsetAsync(r.tile, 0, kRhTileStride * ntiles * sizeof(uint64_t), s));
        hipLaunchKernelGGL(k_rh_size, grid, dim3(kPartThreads), 0, s, a, r);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_rh_scan, dim3(1), dim3(kPartThreads), 0, s, a, r);
    HIPCHK(hipGetLastError());
    if (n_hashes) {
        hipLaunchKernelGGL(k_rh_gather, grid, dim3(kPartThreads), 0, s, a, r);
        HIPCHK(hipGetLastError());
        // (the hashes with several objects: nearly always a word a tile)
        hipLaunchKernelGGL(k_rh_several, grid, dim3(kPartThreads), 0, s, a, r);
        HIPCHK(hipGetLastError());
    }
    return RAMCRC_OK;
}

int ramcrc_replay_table_enumerate_device(ramcrc_replay_table* t, uint64_t table_id, uint64_t first_hash,
                                         uint64_t last_hash, uint64_t bucket_index,
                                         uint64_t bucket_next_hash, uint64_t bucket_limit,
                                         const ramcrc_enum_frame* stale, uint32_t n_stale, uint32_t flags,
                                         void* d_payload, uint64_t payload_capacity, uint64_t max_bytes,
                                         ramcrc_enumerate_summary* d_summary, void* stream)
{
    namespace en = ramcrc_en;
    if (!t || (flags & ~RAMCRC_ENUM_KEYS_ONLY) || !d_summary || (payload_capacity && !d_payload) ||
        n_stale > RAMCRC_ENUM_MAX_STALE || (n_stale && !stale))
        return RAMCRC_EINVAL;
    const uint64_t P = reinterpret_cast<uint64_t>(d_payload);
    if ((reinterpret_cast<uint64_t>(d_summary) & 7) || P > UINT64_MAX - payload_capacity)
        return RAMCRC_EINVAL;
    std::lock_guard<std::mutex> lt(t->mu);
    const uint64_t S = t->nslots;
    if (bucket_index > S || (bucket_limit && (bucket_limit < bucket_index || bucket_limit > S)))
        return RAMCRC_EINVAL;
    EnDesc r{};
    // the stale frames travel in the launch descriptor: no copy to order, and
    // the caller's array is free when the call returns
    for (uint32_t k = 0; k < n_stale; k++) {
        memcpy(&r.sel.stale[k], reinterpret_cast<const uint8_t*>(stale) + k * sizeof(*stale), sizeof(*stale));
        if (en::bad_frame(r.sel.stale[k]))
            return RAMCRC_EINVAL;
    }
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch: a line for the scan's words to the gather, then the tile sums,
    // in the chunk-partial buffer; nothing per bucket (ramcrc.h states this
    // size)
    const uint64_t nb = (bucket_limit ? bucket_limit : S) - bucket_index;
    const uint64_t ntiles = (nb + kPartThreads - 1) / kPartThreads;
    int rc = reserve_locked(c, kLookCountWords + 2 * kEnTileStride * ntiles, 0);
    if (rc)
        return rc;
    const RtabDesc a = rtab_desc(t);
    r.table_id = table_id;
    r.nb = nb;
    r.payload = P;
    r.lim = en::limit(max_bytes, payload_capacity);
    r.summary = d_summary;
    r.flags = flags;
    r.sel.first_hash = first_hash;
    r.sel.last_hash = last_hash;
    r.sel.bucket_index = bucket_index;
    r.sel.bucket_next_hash = bucket_next_hash;
    r.sel.n_stale = n_stale;
    r.head = reinterpret_cast<unsigned long long*>(c->partials);
    r.tile = reinterpret_cast<uint64_t*>(c->partials + kLookCountWords);
    const dim3 grid(rtab_grid(c, nb, kPartThreads));
    if (nb) {
        HIPCHK(hipMemsetAsync(r.tile, 0, kEnTileStride * ntiles * sizeof(uint64_t), s));
        hipLaunchKernelGGL(k_en_size, grid, dim3(kPartThreads), 0, s, a, r);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_en_scan, dim3(1), dim3(kPartThreads), 0, s, a, r);
    HIPCHK(hipGetLastError());
    if (nb) {
        hipLaunchKernelGGL(k_en_gather, grid, dim3(kPartThreads), 0, s, a, r);
        HIPCHK(hipGetLastError());
    }
    return RAMCRC_OK;
}

int ramcrc_replay_table_index_build_device(ramcrc_replay_table* t, uint64_t table_id, uint32_t index_id,
                                           ramcrc_index_entry* d_entries, uint64_t entry_capacity,
                                           uint64_t* d_hashes, void* d_index_keys, uint64_t keys_capacity,
                                           ramcrc_index_build_summary* d_summary, void* stream)
{
    if (!t || !d_summary || index_id == 0 || entry_capacity >= 0xFFFFFFFFull ||
        (entry_capacity && (!d_entries || !d_hashes)) || (keys_capacity && !d_index_keys))
        return RAMCRC_EINVAL;
    const uint64_t K = reinterpret_cast<uint64_t>(d_index_keys);
    if ((reinterpret_cast<uint64_t>(d_entries) & 15) || (reinterpret_cast<uint64_t>(d_hashes) & 7) ||
        (reinterpret_cast<uint64_t>(d_summary) & 7) || K > UINT64_MAX - keys_capacity)
        return RAMCRC_EINVAL;
    std::lock_guard<std::mutex> lt(t->mu);
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch: a line for the scan's words to the later launches, then the
    // tile sums of the slots, in the chunk-partial buffer; the merge passes'
    // second buffer in the plan buffer, when there is a merge pass (ramcrc.h
    // states these sizes)
    const uint64_t ntiles = (t->nslots + kPartThreads - 1) / kPartThreads;
    uint32_t passes = 0;
    for (uint64_t W = kIxTile; W < entry_capacity; W *= 2)
        passes++;
    int rc = reserve_locked(c, kLookCountWords + 2 * kIxTileStride * ntiles, passes ? 4 * entry_capacity : 0);
    if (rc)
        return rc;
    const RtabDesc a = rtab_desc(t);
    IxDesc r{};
    r.table_id = table_id;
    r.index_id = index_id;
    r.entries = d_entries;
    r.ecap = entry_capacity;
    r.hashes = d_hashes;
    r.keys = K;
    r.kcap = keys_capacity;
    r.summary = d_summary;
    r.head = reinterpret_cast<unsigned long long*>(c->partials);
    r.tile = reinterpret_cast<uint64_t*>(c->partials + kLookCountWords);
    HIPCHK(hipMemsetAsync(c->partials, 0,
                          kLookCountWords * sizeof(uint32_t) + kIxTileStride * ntiles * sizeof(uint64_t), s));
    const dim3 grid(rtab_grid(c, t->nslots, kPartThreads));
    hipLaunchKernelGGL(k_ix_size, grid, dim3(kPartThreads), 0, s, a, r);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_ix_scan, dim3(1), dim3(kPartThreads), 0, s, a, r);
    HIPCHK(hipGetLastError());
    if (entry_capacity == 0)
        return RAMCRC_OK;
    hipLaunchKernelGGL(k_ix_emit, grid, dim3(kPartThreads), 0, s, a, r);
    HIPCHK(hipGetLastError());
    // the tile sort leaves its output where an even number of passes ends in d_entries
    ramcrc_index_entry* const other = reinterpret_cast<ramcrc_index_entry*>(c->plan_local);
    ramcrc_index_entry* src = (passes & 1) ? other : d_entries;
    const dim3 sgrid(rtab_grid(c, entry_capacity, kIxTile));
    hipLaunchKernelGGL(k_ix_sort, sgrid, dim3(kPartThreads), 0, s, a, r, src);
    HIPCHK(hipGetLastError());
    for (uint64_t W = kIxTile; W < entry_capacity; W *= 2) {
        ramcrc_index_entry* const dst = src == other ? d_entries : other;
        hipLaunchKernelGGL(k_ix_merge, sgrid, dim3(kPartThreads), 0, s, a, r, W, src, dst);
        HIPCHK(hipGetLastError());
        src = dst;
    }
    hipLaunchKernelGGL(k_ix_hashes, dim3(rtab_grid(c, entry_capacity, kPartThreads)), dim3(kPartThreads), 0, s,
                       a, r);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

int ramcrc_index_lookup_device(ramcrc_ctx* c, const ramcrc_index_entry* d_entries, const uint64_t* d_hashes,
                               const void* d_index_keys, const ramcrc_index_build_summary* d_build_summary,
                               const void* d_qkeys, uint64_t qkeys_bytes, const ramcrc_index_query* d_queries,
                               uint64_t n_queries, uint64_t* d_out_hashes, uint64_t out_capacity,
                               ramcrc_index_result* d_results, ramcrc_index_lookup_summary* d_summary,
                               void* stream)
{
    if (!c || !d_build_summary || !d_summary || n_queries >= 0xFFFFFFFFull ||
        (n_queries && (!d_queries || !d_results)) || (qkeys_bytes && !d_qkeys) ||
        (out_capacity && !d_out_hashes))
        return RAMCRC_EINVAL;
    const uint64_t Q = reinterpret_cast<uint64_t>(d_qkeys);
    if ((reinterpret_cast<uint64_t>(d_entries) & 15) || (reinterpret_cast<uint64_t>(d_hashes) & 7) ||
        (reinterpret_cast<uint64_t>(d_build_summary) & 7) || (reinterpret_cast<uint64_t>(d_queries) & 7) ||
        (reinterpret_cast<uint64_t>(d_out_hashes) & 7) || (reinterpret_cast<uint64_t>(d_results) & 7) ||
        (reinterpret_cast<uint64_t>(d_summary) & 7) || Q > UINT64_MAX - qkeys_bytes)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch: a line for the scan's word to the copy, then the tile sums, in
    // the chunk-partial buffer; two words a query in the plan buffer
    // (ramcrc.h states these sizes)
    const uint64_t ntiles = (n_queries + kPartThreads - 1) / kPartThreads;
    int rc = reserve_locked(c, kLookCountWords + 2 * kIxTileStride * ntiles, 2 * n_queries);
    if (rc)
        return rc;
    IxlDesc r{};
    r.entries = d_entries;
    r.hashes = d_hashes;
    r.keys = reinterpret_cast<uint64_t>(d_index_keys);
    r.build = d_build_summary;
    r.qkeys = Q;
    r.qkeys_bytes = qkeys_bytes;
    r.queries = reinterpret_cast<const uint64_t*>(d_queries);
    r.nq = n_queries;
    r.out = d_out_hashes;
    r.ocap = out_capacity;
    r.results = d_results;
    r.summary = d_summary;
    r.rec = c->plan_local;
    r.head = reinterpret_cast<unsigned long long*>(c->partials);
    r.tile = reinterpret_cast<uint64_t*>(c->partials + kLookCountWords);
    const dim3 grid(rtab_grid(c, n_queries, kPartThreads));
    HIPCHK(hipMemsetAsync(c->partials, 0,
                          kLookCountWords * sizeof(uint32_t) + kIxTileStride * ntiles * sizeof(uint64_t), s));
    if (n_queries) {
        hipLaunchKernelGGL(k_ixl_search, grid, dim3(kPartThreads), 0, s, r);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ixl_scan, dim3(1), dim3(kPartThreads), 0, s, r);
    HIPCHK(hipGetLastError());
    if (n_queries) {
        hipLaunchKernelGGL(k_ixl_copy, grid, dim3(kPartThreads), 0, s, r);
        HIPCHK(hipGetLastError());
        // (the wide ranges: a grid for the output, not for the queries)
        hipLaunchKernelGGL(k_ixl_long, dim3(rtab_grid(c, out_capacity, kPartThreads)), dim3(kPartThreads), 0, s, r);
        HIPCHK(hipGetLastError());
    }
    return RAMCRC_OK;
}

int ramcrc_replay_table_write_device(ramcrc_replay_table* t, const void* d_data, uint64_t data_bytes,
                                     const ramcrc_write_req* d_reqs, uint64_t n_reqs,
                                     const uint64_t* d_key_hash, const ramcrc_reject_rules* d_rules,
                                     uint64_t next_version, uint32_t timestamp,
                                     const uint64_t* d_batch_segment_id, void* d_out,
                                     uint32_t out_capacity, ramcrc_seg_cert* d_out_cert, void* d_parts,
                                     ramcrc_write_ref* d_refs, ramcrc_lookup_result* d_old,
                                     ramcrc_write_summary* d_summary, void* stream)
{
    if (!t || next_version == 0 || n_reqs >= 0xFFFFFFFFull || !d_summary || !d_out_cert ||
        (n_reqs && (!d_reqs || !d_parts)) || (data_bytes && !d_data) || (out_capacity && !d_out))
        return RAMCRC_EINVAL;
    const uint64_t D = reinterpret_cast<uint64_t>(d_data), O = reinterpret_cast<uint64_t>(d_out);
    if ((reinterpret_cast<uint64_t>(d_reqs) & 7) || (reinterpret_cast<uint64_t>(d_key_hash) & 7) ||
        (reinterpret_cast<uint64_t>(d_rules) & 7) || (reinterpret_cast<uint64_t>(d_batch_segment_id) & 7) ||
        (reinterpret_cast<uint64_t>(d_out_cert) & 3) || (reinterpret_cast<uint64_t>(d_parts) & 3) ||
        (reinterpret_cast<uint64_t>(d_refs) & 7) || (reinterpret_cast<uint64_t>(d_old) & 15) ||
        (reinterpret_cast<uint64_t>(d_summary) & 7) || D > UINT64_MAX - data_bytes ||
        O > UINT64_MAX - out_capacity)
        return RAMCRC_EINVAL;
    std::lock_guard<std::mutex> lt(t->mu);
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch: the head line, then the tile sums, in the chunk-partial buffer;
    // the per-request words, then the grouping table, in the plan buffer
    // (ramcrc.h states these sizes)
    const uint64_t ntiles = (n_reqs + kPartThreads - 1) / kPartThreads;
    const uint64_t gslots = ramcrc_res::slots_for(n_reqs);
    int rc = reserve_locked(c, 2 * kWrHeadWords + 2 * kWrTileWords * ntiles, kWrReqWords * n_reqs + 2 * gslots);
    if (rc)
        return rc;
    const RtabDesc a = rtab_desc(t);
    WrDesc w{};
    w.data = D;
    w.data_bytes = data_bytes;
    w.reqs = reinterpret_cast<const uint64_t*>(d_reqs);
    w.nq = n_reqs;
    w.key_hash = d_key_hash;
    w.rules = reinterpret_cast<const uint64_t*>(d_rules);
    w.batch_seg = d_batch_segment_id;
    w.next_version = next_version;
    w.timestamp = timestamp;
    w.cap = out_capacity;
    w.out = O;
    w.cert = d_out_cert;
    w.parts = static_cast<uint32_t*>(d_parts);
    w.refs = reinterpret_cast<uint2*>(d_refs);
    w.summary = d_summary;
    w.query = c->plan_local;
    w.slot = w.query + 3 * n_reqs;
    w.rec = w.slot + n_reqs;
    w.group = reinterpret_cast<unsigned long long*>(w.rec + 4 * n_reqs);
    w.gslots = gslots;
    w.head = reinterpret_cast<unsigned long long*>(c->partials);
    w.tile = reinterpret_cast<uint64_t*>(c->partials + 2 * kWrHeadWords);
    LookDesc q{};
    q.keys = D;
    q.keys_bytes = data_bytes;
    q.queries = w.query;
    q.nq = n_reqs;
    q.key_hash = d_key_hash;
    q.results = reinterpret_cast<u32x4*>(d_old);
    const dim3 grid(rtab_grid(c, n_reqs, kPartThreads));
    HIPCHK(hipMemsetAsync(w.head, 0, (2 * kWrHeadWords + 2 * kWrTileWords * ntiles) * sizeof(uint32_t), s));
    if (n_reqs) {
        HIPCHK(hipMemsetAsync(w.group, 0, 2 * gslots * sizeof(uint64_t), s));
        if (d_key_hash) {
            hipLaunchKernelGGL(k_wr_group<true>, grid, dim3(kPartThreads), 0, s, a, w);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_wr_size<true>, grid, dim3(kPartThreads), 0, s, a, q, w);
        } else {
            hipLaunchKernelGGL(k_wr_group<false>, grid, dim3(kPartThreads), 0, s, a, w);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_wr_size<false>, grid, dim3(kPartThreads), 0, s, a, q, w);
        }
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_wr_scan, dim3(1), dim3(kPartThreads), 0, s, a, w);
    HIPCHK(hipGetLastError());
    // (at least one workgroup: an empty call still gets its certificate)
    hipLaunchKernelGGL(k_wr_emit, grid, dim3(kPartThreads), 0, s, a, w);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

int ramcrc_replay_table_remove_device(ramcrc_replay_table* t, const void* d_keys, uint64_t keys_bytes,
                                      const ramcrc_lookup_key* d_reqs, uint64_t n_reqs,
                                      const uint64_t* d_key_hash, const ramcrc_reject_rules* d_rules,
                                      uint64_t next_version, uint32_t timestamp,
                                      const uint64_t* d_batch_segment_id, void* d_out,
                                      uint32_t out_capacity, ramcrc_seg_cert* d_out_cert, void* d_parts,
                                      uint32_t* d_refs, ramcrc_lookup_result* d_old,
                                      ramcrc_remove_summary* d_summary, void* stream)
{
    if (!t || next_version == 0 || n_reqs >= 0xFFFFFFFFull || !d_summary || !d_out_cert ||
        (n_reqs && (!d_reqs || !d_parts)) || (keys_bytes && !d_keys) || (out_capacity && !d_out))
        return RAMCRC_EINVAL;
    const uint64_t K = reinterpret_cast<uint64_t>(d_keys), O = reinterpret_cast<uint64_t>(d_out);
    if ((reinterpret_cast<uint64_t>(d_reqs) & 7) || (reinterpret_cast<uint64_t>(d_key_hash) & 7) ||
        (reinterpret_cast<uint64_t>(d_rules) & 7) || (reinterpret_cast<uint64_t>(d_batch_segment_id) & 7) ||
        (reinterpret_cast<uint64_t>(d_out_cert) & 3) || (reinterpret_cast<uint64_t>(d_parts) & 3) ||
        (reinterpret_cast<uint64_t>(d_refs) & 3) || (reinterpret_cast<uint64_t>(d_old) & 15) ||
        (reinterpret_cast<uint64_t>(d_summary) & 7) || K > UINT64_MAX - keys_bytes ||
        O > UINT64_MAX - out_capacity)
        return RAMCRC_EINVAL;
    std::lock_guard<std::mutex> lt(t->mu);
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch: the head line, then the tile sums, in the chunk-partial buffer;
    // the per-request words, then the grouping table, in the plan buffer
    // (ramcrc.h states these sizes)
    const uint64_t ntiles = (n_reqs + kPartThreads - 1) / kPartThreads;
    const uint64_t gslots = ramcrc_res::slots_for(n_reqs);
    int rc = reserve_locked(c, 2 * kRmHeadWords + 2 * kRmTileWords * ntiles, kRmReqWords * n_reqs + gslots);
    if (rc)
        return rc;
    const RtabDesc a = rtab_desc(t);
    RmDesc w{};
    w.keys = K;
    w.keys_bytes = keys_bytes;
    w.reqs = reinterpret_cast<const uint64_t*>(d_reqs);
    w.nq = n_reqs;
    w.key_hash = d_key_hash;
    w.rules = reinterpret_cast<const uint64_t*>(d_rules);
    w.batch_seg = d_batch_segment_id;
    w.next_version = next_version;
    w.timestamp = timestamp;
    w.cap = out_capacity;
    w.out = O;
    w.cert = d_out_cert;
    w.parts = static_cast<uint32_t*>(d_parts);
    w.refs = d_refs;
    w.summary = d_summary;
    w.hash = c->plan_local;
    w.slot = w.hash + n_reqs;
    w.rec = w.slot + n_reqs;
    w.group = reinterpret_cast<unsigned long long*>(w.rec + 3 * n_reqs);
    w.gslots = gslots;
    w.head = reinterpret_cast<unsigned long long*>(c->partials);
    w.tile = reinterpret_cast<uint64_t*>(c->partials + 2 * kRmHeadWords);
    // the probe runs over the caller's own requests, with the group pass's
    // hashes as the given ones
    LookDesc q{};
    q.keys = K;
    q.keys_bytes = keys_bytes;
    q.queries = w.reqs;
    q.nq = n_reqs;
    q.key_hash = w.hash;
    q.results = reinterpret_cast<u32x4*>(d_old);
    const dim3 grid(rtab_grid(c, n_reqs, kPartThreads));
    HIPCHK(hipMemsetAsync(w.head, 0, (2 * kRmHeadWords + 2 * kRmTileWords * ntiles) * sizeof(uint32_t), s));
    if (n_reqs) {
        HIPCHK(hipMemsetAsync(w.group, 0, gslots * sizeof(uint64_t), s));
        if (d_key_hash)
            hipLaunchKernelGGL(k_rm_group<true>, grid, dim3(kPartThreads), 0, s, a, w);
        else
            hipLaunchKernelGGL(k_rm_group<false>, grid, dim3(kPartThreads), 0, s, a, w);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_rm_size, grid, dim3(kPartThreads), 0, s, a, q, w);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_rm_scan, dim3(1), dim3(kPartThreads), 0, s, a, w);
    HIPCHK(hipGetLastError());
    // (at least one workgroup: an empty call still gets its certificate)
    hipLaunchKernelGGL(k_rm_emit, grid, dim3(kPartThreads), 0, s, a, w);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

int ramcrc_replay_table_increment_device(ramcrc_replay_table* t, const void* d_keys, uint64_t keys_bytes,
                                         const ramcrc_lookup_key* d_reqs, uint64_t n_reqs,
                                         const ramcrc_increment_arg* d_args,
                                         const uint64_t* d_key_hash, const ramcrc_reject_rules* d_rules,
                                         uint64_t next_version, uint32_t timestamp,
                                         const uint64_t* d_batch_segment_id, void* d_out,
                                         uint32_t out_capacity, ramcrc_seg_cert* d_out_cert, void* d_parts,
                                         ramcrc_write_ref* d_refs, ramcrc_lookup_result* d_old,
                                         ramcrc_increment_summary* d_summary, void* stream)
{
    if (!t || next_version == 0 || n_reqs >= 0xFFFFFFFFull || !d_summary || !d_out_cert ||
        (n_reqs && (!d_reqs || !d_args || !d_parts)) || (keys_bytes && !d_keys) || (out_capacity && !d_out))
        return RAMCRC_EINVAL;
    const uint64_t K = reinterpret_cast<uint64_t>(d_keys), O = reinterpret_cast<uint64_t>(d_out);
    if ((reinterpret_cast<uint64_t>(d_reqs) & 7) || (reinterpret_cast<uint64_t>(d_args) & 7) ||
        (reinterpret_cast<uint64_t>(d_key_hash) & 7) ||
        (reinterpret_cast<uint64_t>(d_rules) & 7) || (reinterpret_cast<uint64_t>(d_batch_segment_id) & 7) ||
        (reinterpret_cast<uint64_t>(d_out_cert) & 3) || (reinterpret_cast<uint64_t>(d_parts) & 3) ||
        (reinterpret_cast<uint64_t>(d_refs) & 7) || (reinterpret_cast<uint64_t>(d_old) & 15) ||
        (reinterpret_cast<uint64_t>(d_summary) & 7) || K > UINT64_MAX - keys_bytes ||
        O > UINT64_MAX - out_capacity)
        return RAMCRC_EINVAL;
    std::lock_guard<std::mutex> lt(t->mu);
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch: the head line, k_wr_scan's summary, then the tile sums, in the
    // chunk-partial buffer; the per-request words, then the grouping table, in
    // the plan buffer (ramcrc.h states these sizes)
    const uint64_t ntiles = (n_reqs + kPartThreads - 1) / kPartThreads;
    const uint64_t gslots = ramcrc_res::slots_for(n_reqs);
    const uint64_t head_words = 2 * kWrHeadWords + kIncSumWords;
    int rc = reserve_locked(c, head_words + 2 * kWrTileWords * ntiles, kIncReqWords * n_reqs + gslots);
    if (rc)
        return rc;
    const RtabDesc a = rtab_desc(t);
    // the group pass is the remove's, over the remove's request layout
    RmDesc r{};
    r.keys = K;
    r.keys_bytes = keys_bytes;
    r.reqs = reinterpret_cast<const uint64_t*>(d_reqs);
    r.nq = n_reqs;
    r.key_hash = d_key_hash;
    r.rules = reinterpret_cast<const uint64_t*>(d_rules);
    r.hash = c->plan_local;
    r.slot = r.hash + n_reqs;
    r.group = reinterpret_cast<unsigned long long*>(r.slot + 6 * n_reqs);
    r.gslots = gslots;
    // the records, the scan and the entries are the write's; the key buffer is its data
    WrDesc w{};
    w.data = K;
    w.data_bytes = keys_bytes;
    w.reqs = r.reqs;
    w.nq = n_reqs;
    w.key_hash = d_key_hash;
    w.rules = r.rules;
    w.batch_seg = d_batch_segment_id;
    w.next_version = next_version;
    w.timestamp = timestamp;
    w.cap = out_capacity;
    w.out = O;
    w.cert = d_out_cert;
    w.parts = static_cast<uint32_t*>(d_parts);   // five words each
    w.refs = reinterpret_cast<uint2*>(d_refs);
    w.summary = reinterpret_cast<ramcrc_write_summary*>(c->partials + 2 * kWrHeadWords);
    w.slot = r.slot;
    w.rec = r.slot + n_reqs;
    w.group = r.group;   // one word a slot
    w.gslots = gslots;
    w.head = reinterpret_cast<unsigned long long*>(c->partials);
    w.tile = reinterpret_cast<uint64_t*>(c->partials + head_words);
    IncDesc x{};
    x.args = reinterpret_cast<const uint64_t*>(d_args);
    x.bits = w.rec + 4 * n_reqs;
    x.summary = d_summary;
    // the probe runs over the caller's own requests, with the group pass's
    // hashes as the given ones
    LookDesc q{};
    q.keys = K;
    q.keys_bytes = keys_bytes;
    q.queries = w.reqs;
    q.nq = n_reqs;
    q.key_hash = r.hash;
    q.results = reinterpret_cast<u32x4*>(d_old);
    const dim3 grid(rtab_grid(c, n_reqs, kPartThreads));
    HIPCHK(hipMemsetAsync(w.head, 0, (head_words + 2 * kWrTileWords * ntiles) * sizeof(uint32_t), s));
    if (n_reqs) {
        HIPCHK(hipMemsetAsync(w.group, 0, gslots * sizeof(uint64_t), s));
        if (d_key_hash)
            hipLaunchKernelGGL(k_rm_group<true>, grid, dim3(kPartThreads), 0, s, a, r);
        else
            hipLaunchKernelGGL(k_rm_group<false>, grid, dim3(kPartThreads), 0, s, a, r);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_inc_size, grid, dim3(kPartThreads), 0, s, a, q, w, x);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_wr_scan, dim3(1), dim3(kPartThreads), 0, s, a, w);
    HIPCHK(hipGetLastError());
    // (at least one workgroup: an empty call still gets its certificate and summary)
    hipLaunchKernelGGL(k_inc_emit, grid, dim3(kPartThreads), 0, s, a, w, x);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

namespace {
// clean and clean_size: out == nullptr is the size form.
struct CleanOut {
    void* out;
    uint32_t cap;
    ramcrc_seg_cert* cert;
    ramcrc_seg_status* status;
    ramcrc_seg_entry* entries;
    uint64_t ecap;
    uint64_t* n_entries;
    uint64_t* work;
    ramcrc_replay_ref* moved;
    uint32_t* batch;
};

int clean_impl(ramcrc_replay_table* t, const uint32_t* victims, uint32_t n_victims, const CleanOut* o,
               ramcrc_clean_usage* d_usage, ramcrc_clean_summary* d_summary, void* stream)
{
    if (!t || !victims || !d_summary || n_victims == 0)
        return RAMCRC_EINVAL;
    if ((reinterpret_cast<uint64_t>(d_usage) & 7) || (reinterpret_cast<uint64_t>(d_summary) & 7))
        return RAMCRC_EINVAL;
    if (o) {
        const uint64_t O = reinterpret_cast<uint64_t>(o->out);
        if (!o->cert || !o->status || !o->n_entries || (o->ecap && (!o->entries || !o->work)) ||
            (o->cap && !o->out) || (O & 15) || (o->cap & 15) || o->ecap >= 0x100000000ull ||
            O > UINT64_MAX - o->cap || (reinterpret_cast<uint64_t>(o->cert) & 3) ||
            (reinterpret_cast<uint64_t>(o->status) & 3) || (reinterpret_cast<uint64_t>(o->entries) & 15) ||
            (reinterpret_cast<uint64_t>(o->n_entries) & 7) || (reinterpret_cast<uint64_t>(o->work) & 7) ||
            (reinterpret_cast<uint64_t>(o->moved) & 7))
            return RAMCRC_EINVAL;
    }
    std::lock_guard<std::mutex> lt(t->mu);
    if (o && t->ecap.size() >= t->max_batches)
        return RAMCRC_EINVAL;
    // the victims: numbered, not cleaned, none twice; their tiles
    std::vector<uint64_t> vic;
    uint64_t ntiles = 0;
    try {
        std::vector<uint8_t> seen(t->ecap.size(), 0);
        vic.reserve(uint64_t(n_victims) + 1);
        for (uint32_t v = 0; v < n_victims; v++) {
            const uint32_t b = victims[v];
            if (b >= t->ecap.size() || t->retired[b] || seen[b])
                return RAMCRC_EINVAL;
            seen[b] = 1;
            vic.push_back((uint64_t(b) << 48) | ntiles);
            ntiles += (t->ecap[b] + kPartThreads - 1) / kPartThreads;
        }
        vic.push_back(ntiles);
        if (o) {
            t->ecap.reserve(t->ecap.size() + 1);
            t->retired.reserve(t->retired.size() + 1);
        }
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch, in the chunk-partial buffer: the victim list, then a line per
    // tile (ramcrc.h states this size)
    const uint64_t vic_words = (uint64_t(n_victims) + 1 + 15) & ~15ull;
    int rc = reserve_locked(c, 2 * (uint64_t(n_victims) + 16 + kClTileWords * ntiles), 0);
    if (rc)
        return rc;
    RtabDesc a = rtab_desc(t);
    ClDesc d{};
    d.nvic = n_victims;
    d.ntiles = ntiles;
    uint64_t* const d_vic = reinterpret_cast<uint64_t*>(c->partials);
    d.vic = d_vic;
    d.tile = d_vic + vic_words;
    d.size_only = o ? 0u : 1u;
    d.usage = d_usage;
    d.summary = d_summary;
    // the list travels in the kernels' arguments: the call stays capturable
    // and no host memory has to outlive it
    for (uint64_t f = 0; f < vic.size(); f += kClOpenMax) {
        ClOpen op;
        op.vic = d_vic;
        op.first = f;
        op.n = uint32_t(vic.size() - f < kClOpenMax ? vic.size() - f : kClOpenMax);
        memcpy(op.w, vic.data() + f, op.n * sizeof(uint64_t));
        hipLaunchKernelGGL(k_clean_open, dim3(1), dim3(kClOpenMax), 0, s, op);
        HIPCHK(hipGetLastError());
    }
    if (o) {
        d.survivor = a.batch = uint32_t(t->ecap.size());
        d.out = reinterpret_cast<uint64_t>(o->out);
        d.cap = o->cap;
        d.ecap = o->ecap;
        d.cert = o->cert;
        d.status = o->status;
        d.entries = reinterpret_cast<u32x4*>(o->entries);
        d.n_entries = o->n_entries;
        d.work = o->work;
        d.moved = reinterpret_cast<uint2*>(o->moved);
        // the survivor is a batch of the table from here on
        a.open.base = d.out;
        a.open.stride = o->cap;
        a.open.nseg = 1;
        a.open.status = o->status;
        a.open.entries = reinterpret_cast<const u32x4*>(o->entries);
        a.open.n_entries = o->n_entries;
        a.open.ecap = o->ecap;
        a.open.key_hash = nullptr;   // nothing reads a batch's hashes after its insert
        a.open.work = o->work;
        hipLaunchKernelGGL(k_rtab_open, dim3(1), dim3(kWaveSize), 0, s, a);
        HIPCHK(hipGetLastError());
        // the number is taken and the victims are retired whatever the device finds
        t->ecap.push_back(o->ecap);
        t->retired.push_back(0);
        for (uint32_t v = 0; v < n_victims; v++)
            t->retired[victims[v]] = 1;
        if (o->batch)
            *o->batch = d.survivor;
    }
    const dim3 grid(rtab_grid(c, ntiles * kPartThreads, kPartThreads));
    hipLaunchKernelGGL(k_clean_mark, grid, dim3(kPartThreads), 0, s, a, d);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_clean_scan, dim3(1), dim3(kPartThreads), 0, s, a, d);
    HIPCHK(hipGetLastError());
    if (o) {
        hipLaunchKernelGGL(k_clean_move, grid, dim3(kPartThreads), 0, s, a, d);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_clean_claims, grid, dim3(kPartThreads), 0, s, a, d);
        HIPCHK(hipGetLastError());
    }
    return RAMCRC_OK;
}
}  // namespace

int ramcrc_replay_table_clean_size_device(ramcrc_replay_table* t, const uint32_t* victims,
                                          uint32_t n_victims, ramcrc_clean_usage* d_usage,
                                          ramcrc_clean_summary* d_summary, void* stream)
{
    return clean_impl(t, victims, n_victims, nullptr, d_usage, d_summary, stream);
}

int ramcrc_replay_table_clean_device(ramcrc_replay_table* t, const uint32_t* victims, uint32_t n_victims,
                                     void* d_out, uint32_t out_capacity, ramcrc_seg_cert* d_out_cert,
                                     ramcrc_seg_status* d_out_status, ramcrc_seg_entry* d_out_entries,
                                     uint64_t out_entries_cap, uint64_t* d_out_n_entries,
                                     uint64_t* d_out_work, ramcrc_replay_ref* d_moved,
                                     ramcrc_clean_usage* d_usage, ramcrc_clean_summary* d_summary,
                                     uint32_t* batch, void* stream)
{
    const CleanOut o{d_out, out_capacity, d_out_cert, d_out_status, d_out_entries, out_entries_cap,
                     d_out_n_entries, d_out_work, d_moved, batch};
    return clean_impl(t, victims, n_victims, &o, d_usage, d_summary, stream);
}

int ramcrc_replay_table_migrate_device(ramcrc_replay_table* t, const uint32_t* batches, uint32_t n_batches,
                                       uint64_t table_id, uint64_t first_hash, uint64_t last_hash,
                                       uint32_t flags, uint32_t start_index, uint32_t start_record,
                                       void* d_out, uint32_t out_capacity, uint64_t out_stride,
                                       uint32_t max_segments, ramcrc_seg_cert* d_out_certs,
                                       ramcrc_migrate_count* d_out_counts, ramcrc_replay_ref* d_sent,
                                       uint64_t sent_cap, uint64_t* d_seg_first,
                                       ramcrc_migrate_summary* d_summary, void* stream)
{
    if (!t || !batches || !d_summary || n_batches == 0 || (flags & ~ramcrc_mig::kKnownFlags))
        return RAMCRC_EINVAL;
    const uint64_t O = reinterpret_cast<uint64_t>(d_out);
    if ((reinterpret_cast<uint64_t>(d_summary) & 7) || (O & 15) || (out_capacity & 15) || (out_stride & 15) ||
        out_stride < out_capacity || out_capacity > RAMCRC_MIGRATE_MAX_CAPACITY ||
        max_segments > RAMCRC_MIGRATE_MAX_SEGMENTS ||
        (max_segments && (!d_out_certs || !d_out_counts || (out_capacity && !d_out))) ||
        (out_stride && max_segments > (UINT64_MAX - O) / out_stride) ||
        (reinterpret_cast<uint64_t>(d_out_certs) & 3) || (reinterpret_cast<uint64_t>(d_out_counts) & 3) ||
        (reinterpret_cast<uint64_t>(d_sent) & 7) || (reinterpret_cast<uint64_t>(d_seg_first) & 7) ||
        (sent_cap && !d_sent) || start_index > n_batches || (start_index == n_batches && start_record))
        return RAMCRC_EINVAL;
    std::lock_guard<std::mutex> lt(t->mu);
    // the list: numbered, not cleaned, none twice; the tiles from the cursor on
    std::vector<uint64_t> list;
    uint64_t ntiles = 0;
    try {
        std::vector<uint8_t> seen(t->ecap.size(), 0);
        list.reserve(uint64_t(n_batches) + 1);
        for (uint32_t v = 0; v < n_batches; v++) {
            const uint32_t b = batches[v];
            if (b >= t->ecap.size() || t->retired[b] || seen[b])
                return RAMCRC_EINVAL;
            seen[b] = 1;
            if (v < start_index)
                continue;
            uint64_t n = t->ecap[b];
            if (v == start_index) {
                if (start_record > n)
                    return RAMCRC_EINVAL;
                n -= uint64_t(start_record) & ~uint64_t(kPartThreads - 1);
            }
            list.push_back((uint64_t(b) << 48) | ntiles);
            ntiles += (n + kPartThreads - 1) / kPartThreads;
        }
        list.push_back(ntiles);
    } catch (...) {
        return RAMCRC_ENOMEM;
    }
    if (ntiles > kClFirstMask)
        return RAMCRC_EINVAL;
    ramcrc_ctx* c = t->ctx;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // scratch, in the chunk-partial buffer: the list, the head line, the
    // boundaries, a line per tile; in the plan buffer a word per record
    // (ramcrc.h states these sizes)
    const uint64_t list_words = (uint64_t(list.size()) + 15) & ~15ull;
    const uint64_t bound_words = uint64_t(kMgBoundWords) * (uint64_t(max_segments) + 1);
    int rc = reserve_locked(c, 2 * (uint64_t(n_batches) + 40 + 8 * uint64_t(max_segments) + kMgTileWords * ntiles),
                            (kPartThreads / 2) * ntiles);
    if (rc)
        return rc;
    const RtabDesc a = rtab_desc(t);
    MgDesc d{};
    d.nlist = list.size() - 1;
    d.ntiles = ntiles;
    uint64_t* const d_list = reinterpret_cast<uint64_t*>(c->partials);
    d.list = d_list;
    d.head = d_list + list_words;
    d.bound = d.head + kMgHeadWords;
    d.tile = d.bound + bound_words;
    d.rec = reinterpret_cast<uint32_t*>(c->plan_local);
    d.table_id = table_id;
    d.first_hash = first_hash;
    d.last_hash = last_hash;
    d.flags = flags;
    d.start_index = start_index;
    d.start_record = start_record;
    d.n_batches = n_batches;
    d.out = O;
    d.cap = out_capacity;
    d.stride = out_stride;
    d.max_segments = max_segments;
    d.certs = d_out_certs;
    d.counts = d_out_counts;
    d.sent = reinterpret_cast<uint2*>(d_sent);
    d.sent_cap = sent_cap;
    d.seg_first = d_seg_first;
    d.summary = d_summary;
    // the list travels in the kernels' arguments, as clean's does
    for (uint64_t f = 0; f < list.size(); f += kClOpenMax) {
        ClOpen op;
        op.vic = d_list;
        op.first = f;
        op.n = uint32_t(list.size() - f < kClOpenMax ? list.size() - f : kClOpenMax);
        memcpy(op.w, list.data() + f, op.n * sizeof(uint64_t));
        hipLaunchKernelGGL(k_clean_open, dim3(1), dim3(kClOpenMax), 0, s, op);
        HIPCHK(hipGetLastError());
    }
    const dim3 grid(rtab_grid(c, ntiles * kPartThreads, kPartThreads));
    hipLaunchKernelGGL(k_mig_size, grid, dim3(kPartThreads), 0, s, a, d);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_mig_cut, dim3(1), dim3(kPartThreads), 0, s, a, d);
    HIPCHK(hipGetLastError());
    if (max_segments) {
        hipLaunchKernelGGL(k_mig_emit, grid, dim3(kPartThreads), 0, s, a, d);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_mig_seal, dim3(rtab_grid(c, max_segments, kPartThreads)), dim3(kPartThreads), 0, s,
                           a, d);
        HIPCHK(hipGetLastError());
    }
    return RAMCRC_OK;
}

int ramcrc_verify_objects_device(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride,
                                 const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                 const uint64_t* d_n_entries, uint32_t* d_obj_crc,
                                 ramcrc_seg_status* d_status, void* stream)
{
    if (!c)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    return verify_impl(c, d_base, seg_stride, d_entries, entries_cap, d_n_entries, d_obj_crc,
                       d_status, reinterpret_cast<hipStream_t>(stream), nullptr);
}

namespace {
int verify_impl(ramcrc_ctx* c, const void* d_base, uint64_t seg_stride,
                const ramcrc_seg_entry* d_entries, uint64_t entries_cap, const uint64_t* d_n_entries,
                uint32_t* d_obj_crc, ramcrc_seg_status* d_status, hipStream_t s, const uint32_t* sum,
                uint64_t n_seg)
{
    if (entries_cap == 0)
        return RAMCRC_OK;
    if (!d_base || !d_entries || !d_n_entries || !d_obj_crc || !d_status)
        return RAMCRC_EINVAL;
    int rc = reserve_locked(c, default_chunk_bound(entries_cap), entries_cap);
    if (rc)
        return rc;
    BatchDesc d{};
    d.cshift = kChunkShift;
    d.base = static_cast<const uint8_t*>(d_base);
    d.seg_bytes = seg_stride;
    d.n = entries_cap;
    d.vstat = d_status;
    d.rec = reinterpret_cast<const u32x4*>(d_entries);
    d.n_dev = d_n_entries;
    d.seg_status = reinterpret_cast<const u32x4*>(d_status);
    d.out = d_obj_crc;
    d.flags = RAMCRC_FINALIZE;
    if (sum && c->walk_left && !c->serial_walk) {
        // the fused call's verify-in-walk leftovers (exits unless k_walk_probe chose that mode)
        uint64_t gl = uint64_t(4) * c->ncu;
        hipLaunchKernelGGL(k_left, dim3(gl), dim3(256), 0, s, d, d_status, sum, c->walk_left,
                           reinterpret_cast<const unsigned long long*>(c->walk_pool_used + 2),
                           c->walk_left_cap, n_seg);
        HIPCHK(hipGetLastError());
    }
    const uint32_t* nother = nullptr;
    rc = launch_planned<kRecords>(c, d, s, &nother, sum);
    if (rc)
        return rc;
    uint64_t grid = (entries_cap + 255) / 256;
    grid = grid < uint64_t(16) * c->ncu ? grid : uint64_t(16) * c->ncu;
    hipLaunchKernelGGL(k_obj_compare, dim3(grid), dim3(256), 0, s, d, d_status, nother);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}
}  // namespace

int ramcrc_assemble_objects_device(ramcrc_ctx* c, void* d_base, const uint64_t* d_off,
                                   const uint64_t* d_len, uint32_t* d_out, uint64_t n,
                                   void* stream)
{
    if (n == 0)
        return c ? RAMCRC_OK : RAMCRC_EINVAL;
    if (!c || !d_base || !d_off || !d_len)
        return RAMCRC_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc = reserve_locked(c, default_chunk_bound(n), n);
    if (rc)
        return rc;
    if (!d_out) {
        rc = grow_device(reinterpret_cast<void**>(&c->obj_out), &c->obj_out_cap, n,
                         sizeof(uint32_t));
        if (rc)
            return rc;
        d_out = c->obj_out;
    }
    BatchDesc d{};
    d.cshift = kChunkShift;
    d.base = static_cast<const uint8_t*>(d_base);
    d.off = d_off;
    d.len = d_len;
    d.n = n;
    d.out = d_out;
    d.flags = RAMCRC_FINALIZE;
    rc = launch_planned<kObjects>(c, d, s);
    if (rc)
        return rc;
    hipLaunchKernelGGL(k_obj_stamp, dim3((n + 255) / 256), dim3(256), 0, s, d);
    HIPCHK(hipGetLastError());
    return RAMCRC_OK;
}

int ramcrc_assemble_objects_host(ramcrc_ctx* c, void* const* objs, const uint64_t* lens,
                                 uint64_t n)
{
    if (!c || (n && (!objs || !lens)))
        return RAMCRC_EINVAL;
    // CRC of bytes [4, len) of every object with a full header through the
    // pinned-staging batch path, then header.checksum stamped on the host.
    std::vector<const void*> ptrs;
    std::vector<uint64_t> ls;
    std::vector<uint64_t> which;
    for (uint64_t i = 0; i < n; i++) {
        if (lens[i] < kObjHeaderBytes)
            continue;
        if (!objs[i])
            return RAMCRC_EINVAL;
        ptrs.push_back(static_cast<const uint8_t*>(objs[i]) + 4);
        ls.push_back(lens[i] - 4);
        which.push_back(i);
    }
    if (ptrs.empty())
        return RAMCRC_OK;
    std::vector<uint32_t> out(ptrs.size());
    int rc = ramcrc_batch_host(c, ptrs.data(), ls.data(), nullptr, out.data(), ptrs.size(),
                               RAMCRC_FINALIZE);
    if (rc)
        return rc;
    for (size_t k = 0; k < which.size(); k++) {
        uint8_t* p = static_cast<uint8_t*>(objs[which[k]]);
        for (int b = 0; b < 4; b++)
            p[b] = uint8_t(out[k] >> (8 * b));
    }
    return RAMCRC_OK;
}

}  // extern "C"
