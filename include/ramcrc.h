/*
 * ramcrc.h -- the C ABI of the MI355X-native CRC32C path (libramcrc.so).
 *
 * Plain C: no HIP, ROCm or torch types.  Device pointers are `const void*` /
 * `uint32_t*` into memory the caller allocated on the GPU; streams are passed
 * as `void*` (a hipStream_t; NULL = the legacy default stream).
 *
 * Semantics of every CRC entry point follow RAMCloud's Crc32C
 * (/root/reference/src/Crc32C.h):
 *   state 0xFFFFFFFF at construction            (src/Crc32C.h:175-179)
 *   update(p, n): state = CRC32C step, no ~      (src/Crc32C.h:200-206)
 *   getResult():  ~state, state unchanged        (src/Crc32C.h:247-249)
 * The batch entry points compute, for every buffer i,
 *   state_i = init ? init[i] : 0xFFFFFFFF;  state_i = update(buf_i, len_i)
 *   out[i]  = (flags & RAMCRC_FINALIZE) ? ~state_i : state_i
 * i.e. exactly `Crc32C c; c.result = init[i]; c.update(buf_i, len_i);`
 * followed by getResult() or a read of c.result.
 *
 * Errors: every int-returning function returns RAMCRC_OK (0) or a negative
 * code; nothing throws across this boundary.  The reference's update() cannot
 * fail (src/Crc32C.h:200-206); integrity failures stay with the caller, who
 * compares the returned per-buffer CRCs (src/Segment.cc:793-797).
 */
#ifndef RAMCRC_H
#define RAMCRC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    RAMCRC_OK = 0,
    RAMCRC_EINVAL = -1,   /* bad argument (null pointer, size overflow) */
    RAMCRC_ENOMEM = -2,   /* device or pinned allocation failed */
    RAMCRC_EHIP = -3,     /* a HIP runtime call failed; see ramcrc_last_hip_error */
    RAMCRC_ENODEV = -4,   /* no usable gfx950 device */
    RAMCRC_ERCCL = -5,    /* RCCL failure or RCCL unavailable (multi-GPU shard) */
    RAMCRC_EREFUSED = -6, /* a launch found more chunks than the context's scratch holds, or
                             ramcrc_recovery_append_device a placement list it refuses, or
                             ramcrc_recovery_partition_device a tablet list or record table
                             it refuses, or ramcrc_replay_resolve_device a record table it
                             refuses, and wrote none of its outputs (see ramcrc_ctx_check) */
    RAMCRC_EINTERNAL = -7, /* a small-entry launch found its bin layout inconsistent with the
                             entries it binned and wrote none of its small-entry outputs.
                             Only a corrupted bin table produces it (the TEST_DIRTY_BINS
                             hook does so on purpose); scheduling cannot: a one-launch
                             binning whose grid is not all resident (other contexts'
                             kernels, preemption) falls back to the two-launch binning
                             inside the same call.  See ramcrc_ctx_check. */
    RAMCRC_EPEER = -8     /* multi-GPU shard: this rank's part of the step succeeded but
                             another rank's failed; that rank's segments read 0xFFFFFFFF */
    /* -9 was RAMCRC_EORDER of the ordered-stream batches, removed in round 5 */
};

/* Output flag: apply the final inversion (Crc32C::getResult, src/Crc32C.h:247).
 * Without it the raw running state (Crc32C::result, :259) is returned, which
 * callers use to keep chaining (src/LogDigest.cc:75-80, src/Segment.cc:677-681). */
#define RAMCRC_FINALIZE 1u
/* Any other flag bit is RAMCRC_EINVAL.  Round 4's RAMCRC_ORDERED (2) and its
 * ordered entry points were removed in round 5; a caller
 * built against that header gets EINVAL instead of a silently ignored flag.
 * RAMCRC_ABI_VERSION counts such removals. */
#define RAMCRC_ABI_VERSION 6

/* ---------------------------------------------------------------- host --- */

/* Replaces the body of Crc32C::update(const void*, uint32_t)
 * (src/Crc32C.h:200-206) when useHardware: SSE4.2 crc32 instruction,
 * three interleaved streams recombined with X^n operators.  Same result as
 * intelCrc32C (src/Crc32C.h:39-93) for every input.  64-bit length
 * (the reference takes uint32_t; see SURVEY.md section 7, hard part 6). */
uint32_t ramcrc_update_hw(uint32_t state, const void* data, uint64_t nbytes);

/* Replaces softwareCrc32C (src/Crc32C.h:96-153): slicing-by-8, tables
 * generated from the polynomial.  Used when forceSoftware or no SSE4.2. */
uint32_t ramcrc_update_sw(uint32_t state, const void* data, uint64_t nbytes);

/* Best available host path (what Crc32C::update uses by default). */
uint32_t ramcrc_update(uint32_t state, const void* data, uint64_t nbytes);

/* Replaces haveSse42()/Crc32C::haveHardware (src/Crc32C.cc:24-45):
 * 1 if this CPU and build support the crc32 instruction. */
int ramcrc_cpu_has_hw(void);

/* The eight slicing-by-8 tables ramcrc_update_sw uses, 8 x 256 words, table k
 * first: the values of the reference's Crc32CSlicingBy8::crc_tableil8_o32 ..
 * crc_tableil8_o88 (src/Crc32C.h:25-34, src/Crc32C.cc:108-537), generated from
 * the polynomial at compile time.  The drop-in header exposes them under the
 * reference's names. */
const uint32_t* ramcrc_slice8_tables(void);

/* State algebra.  ramcrc_shift(s, n) is the
 * state reached from s by updating with n zero bytes; ramcrc_combine(a, b, n)
 * = raw state of A||B given a = raw(0-based) state after A and b = raw(0, B)
 * with n = |B|.  Both are exact GF(2) identities. */
uint32_t ramcrc_shift(uint32_t state, uint64_t nbytes);
uint32_t ramcrc_combine(uint32_t raw_a, uint32_t raw_b, uint64_t len_b);

/* -------------------------------------------------------------- device --- */

typedef struct ramcrc_ctx ramcrc_ctx;

/* Creates a context bound to HIP device `device` (scratch buffers, pinned
 * staging, device properties).  No GPU work happens at static-init time;
 * contexts are created lazily by callers.  A context serialises its own
 * scratch: use one context per concurrently-launching thread/stream. */
int ramcrc_ctx_create(int device, ramcrc_ctx** out);
int ramcrc_ctx_destroy(ramcrc_ctx* ctx);

/* Pre-size device scratch so later launches never allocate (required before
 * capturing launches into a hipGraph).  max_chunks = number of 256 KiB chunks
 * a launch may cover; max_entries = entries of the largest batch call. */
int ramcrc_ctx_reserve(ramcrc_ctx* ctx, uint64_t max_chunks, uint64_t max_entries);

/* How many times this process has allocated or grown device scratch, over all
 * contexts.  A call "does not allocate" exactly when this count is the same
 * before and after it; tests of the reserve formulas read it. */
int ramcrc_debug_scratch_allocations(uint64_t* count);

/* Uniform contiguous segments (the recovery-scan batch, src/BackupMasterRecovery.cc:743-809
 * per replica): segment i = d_base + i*seg_bytes, i < nseg.  d_init may be NULL.
 * Stream-ordered, asynchronous. */
int ramcrc_segments_device(ramcrc_ctx* ctx, const void* d_base, uint64_t seg_bytes,
                           uint64_t nseg, const uint32_t* d_init, uint32_t* d_out,
                           uint32_t flags, void* stream);

/* General batch: buffer i = d_base + d_off[i], length d_len[i] (64-bit, any
 * alignment, any length including 0).  Buffers of >= 64 KiB are split into
 * 256 KiB chunks scanned by all CUs; smaller ones go to the small-entry
 * kernel.  Stream-ordered, asynchronous. */
int ramcrc_batch_device(ramcrc_ctx* ctx, const void* d_base, const uint64_t* d_off,
                        const uint64_t* d_len, const uint32_t* d_init, uint32_t* d_out,
                        uint64_t n, uint32_t flags, void* stream);

/* Small-entry path only (log entries / objects, src/ObjectManager.cc:659-669):
 * every buffer through the per-entry kernel regardless of length. */
int ramcrc_entries_device(ramcrc_ctx* ctx, const void* d_base, const uint64_t* d_off,
                          const uint64_t* d_len, const uint32_t* d_init, uint32_t* d_out,
                          uint64_t n, uint32_t flags, void* stream);

/* Host buffers in, host CRCs out (segments arriving from disk/NIC buffers,
 * src/BackupStorage.h:227): pinned staging + H2D + kernel + D2H, synchronous.
 * ptrs[i]/lens[i] describe buffer i; init may be NULL. */
int ramcrc_batch_host(ramcrc_ctx* ctx, const void* const* ptrs, const uint64_t* lens,
                      const uint32_t* init, uint32_t* out, uint64_t n, uint32_t flags);

/* Streaming segments host-to-host with H2D on a copy stream overlapped with
 * kernels on a compute stream (BASELINE config 5).  Segment i = h_base +
 * i*seg_bytes (host memory, pinned or pageable); CRCs to h_out.  Uses up to
 * `depth` in-flight device slots of `batch` segments each. */
int ramcrc_stream_host(ramcrc_ctx* ctx, const void* h_base, uint64_t seg_bytes,
                       uint64_t nseg, uint32_t* h_out, uint32_t flags, int batch, int depth);

/* ------------------------------------------- recovery-segment verify --- */

/* SegmentCertificate (src/LogMetadata.h:85-128): 8 bytes, packed. */
typedef struct ramcrc_seg_cert {
    uint32_t segment_length;
    uint32_t checksum;
} ramcrc_seg_cert;

/* One walked log entry (src/Segment.h:99-195): `offset` is the entry's
 * EntryHeader byte within its segment, `header` that byte (type = header &
 * 0x3f, length bytes = ((header >> 6) & 3) + 1) plus RAMCRC_SEG_ENTRY_OVERLONG
 * when the payload would run past the segment capacity (reachable only
 * through the uint32_t offset wrap of the reference's walk), `length` the
 * payload length; the payload starts at offset + 1 + length bytes. */
#define RAMCRC_SEG_ENTRY_OVERLONG 0x100u
typedef struct ramcrc_seg_entry {
    uint32_t segment;
    uint32_t offset;
    uint32_t length;
    uint32_t header;
} ramcrc_seg_entry;

/* Per-segment result of the walk (and of the object verify). */
typedef struct ramcrc_seg_status {
    uint32_t flags;        /* RAMCRC_SEG_* */
    uint32_t checksum;     /* metadata checksum the walk computed (over the entries walked + length) */
    uint32_t entries;      /* entries walked */
    uint32_t bad_objects;  /* replay records whose checksum check failed: objects, tombstones,
                              safe versions and transaction records (see
                              ramcrc_verify_objects_device) */
} ramcrc_seg_status;

#define RAMCRC_SEG_OK 1u              /* Segment::checkMetadataIntegrity returned true */
#define RAMCRC_SEG_PAST_CAPACITY 2u   /* an entry ran past the segment capacity (src/Segment.cc:777-783) */
#define RAMCRC_SEG_PAST_LENGTH 4u     /* entries ran past certificate.segmentLength (:786-790) */
#define RAMCRC_SEG_BAD_CHECKSUM 8u    /* certificate checksum mismatch (:795-797) */
#define RAMCRC_SEG_TABLE_FULL 16u     /* entry table capacity exhausted: records of this segment
                                         were dropped, so it is NOT verified -- RAMCRC_SEG_OK is
                                         never set with this flag and none of its records are
                                         checked; size entries_cap for the smallest entry the
                                         segments can hold and walk again */
#define RAMCRC_SEG_CYCLE 32u          /* the walk revisited an offset (uint32_t wrap): the
                                         reference's loop would not terminate; stopped */
#define RAMCRC_LOG_ENTRY_TYPE_OBJ 2u          /* LOG_ENTRY_TYPE_OBJ, src/LogEntryTypes.h:35 */
#define RAMCRC_LOG_ENTRY_TYPE_OBJTOMB 3u      /* LOG_ENTRY_TYPE_OBJTOMB, src/LogEntryTypes.h:38 */
#define RAMCRC_LOG_ENTRY_TYPE_SAFEVERSION 5u  /* LOG_ENTRY_TYPE_SAFEVERSION, src/LogEntryTypes.h:44 */
#define RAMCRC_LOG_ENTRY_TYPE_PREP 8u         /* LOG_ENTRY_TYPE_PREP, src/LogEntryTypes.h:53 */
#define RAMCRC_LOG_ENTRY_TYPE_PREPTOMB 9u     /* LOG_ENTRY_TYPE_PREPTOMB, src/LogEntryTypes.h:56 */
#define RAMCRC_LOG_ENTRY_TYPE_TXDECISION 10u  /* LOG_ENTRY_TYPE_TXDECISION, src/LogEntryTypes.h:59 */
#define RAMCRC_LOG_ENTRY_TYPE_TXPLIST 11u     /* LOG_ENTRY_TYPE_TXPLIST, src/LogEntryTypes.h:62 */

/* Segment::checkMetadataIntegrity (src/Segment.cc:758-800) for n_seg segments
 * at d_base + i*seg_stride, each of seg_capacity bytes (a multiple of 16; the
 * reference's segletBlocks.size() * segletSize), against d_certs[i].  The
 * length-prefixed entries are walked in parallel over parts of every segment
 * (about 64 entries per part, 64 KiB .. 1 MiB, chosen per batch on the device from
 * the entry density; see RAMCRC_OPT_SERIAL_WALK, RAMCRC_OPT_WALK_PART_SHIFT).  Writes d_status[i] and one
 * ramcrc_seg_entry per complete entry to d_entries (up to entries_cap; the
 * order across segments is unspecified, within a segment it is increasing).
 * The records of one segment are contiguous in the table: segment s owns one
 * run of slots, so a list of record indices that does not decrease visits
 * every segment's records as one run, in offset order
 * (ramcrc_recovery_append_device relies on it).  *d_n_entries (device) receives the
 * number of entries walked (may exceed entries_cap: see TABLE_FULL).
 * d_base 16-byte aligned, seg_stride a multiple of 16.  Stream-ordered. */
int ramcrc_segment_walk_device(ramcrc_ctx* ctx, const void* d_base, uint64_t seg_stride,
                               uint32_t seg_capacity, uint64_t n_seg,
                               const ramcrc_seg_cert* d_certs, ramcrc_seg_status* d_status,
                               ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                               uint64_t* d_n_entries, void* stream);

/* Certificates of rebuilt segments (second half): a
 * backup seals every recovery segment it rebuilt with
 * Segment::getAppendedLength (src/Segment.cc:672-684, called at
 * src/BackupMasterRecovery.cc:367-368 for the segments
 * RecoverySegmentBuilder::build appended, src/RecoverySegmentBuilder.cc:195).
 * For n_seg segments at d_base + i*seg_stride (seg_capacity bytes each, the
 * walk's geometry rules) whose entries were appended from offset 0 up to
 * d_heads[i] (Segment::head), writes d_certs[i] = {head, checksum}: the
 * running Crc32C over every entry's header byte and length bytes, then over
 * the 4 head bytes, finalized -- the metadata the walk covers.  d_flags
 * (nullable) receives RAMCRC_SEG_OK when the entries end exactly at the head,
 * else the walk's RAMCRC_SEG_PAST_CAPACITY / _PAST_LENGTH / _CYCLE findings
 * (the certificate then covers the entries the walk read).  Stream-ordered. */
int ramcrc_segments_certify_device(ramcrc_ctx* ctx, const void* d_base, uint64_t seg_stride,
                                   uint32_t seg_capacity, uint64_t n_seg, const uint32_t* d_heads,
                                   ramcrc_seg_cert* d_certs, uint32_t* d_flags, void* stream);

/* Recovery segments built from walked records: the append loop of
 * RecoverySegmentBuilder::build (src/RecoverySegmentBuilder.cc:61-203) with
 * the placement decision (key hash, tablet lookup) left to the caller.  A
 * placement {record, partition} appends record `record` of the walk table to
 * the recovery segment of `partition` that belongs to the record's source
 * segment; a record may be placed any number of times (the reference places
 * SAFEVERSION and TXPLIST entries in every partition). */
typedef struct ramcrc_placement {
    uint32_t record;     /* index into the walk's record table */
    uint32_t partition;  /* < n_part */
} ramcrc_placement;

typedef struct ramcrc_append_status {
    uint32_t flags;    /* RAMCRC_SEG_OK, RAMCRC_SEG_APPEND_FULL or RAMCRC_SEG_SOURCE_BAD */
    uint32_t entries;  /* entries appended */
} ramcrc_append_status;

#define RAMCRC_SEG_APPEND_FULL 64u   /* a placement did not fit (Segment::hasSpaceFor,
                                        src/Segment.cc:136-154, where the reference throws): it
                                        and every later placement of this output were left out */
#define RAMCRC_SEG_SOURCE_BAD 128u   /* the source segment's status lacks RAMCRC_SEG_OK: nothing
                                        appended (build throws before its loop) */

/* There are n_seg * n_part outputs; output k = s * n_part + p lies at d_out +
 * k * out_stride, holds out_capacity bytes and starts empty (head 0, the
 * running checksum of a fresh Crc32C).  It receives, in list order, every
 * placement {record, p} whose record belongs to source segment s, each as
 * Segment::append(type, payload, length) writes it (src/Segment.cc:197-228):
 * the header byte type | (lengthBytes - 1) << 6 with the minimal lengthBytes
 * for `length` (the EntryHeader constructor, src/Segment.h:134-149 -- not
 * copied from the source header), the length little-endian, the payload.  An
 * append with head + 1 + lengthBytes + length > out_capacity is refused, and
 * so is every later one of that output (RAMCRC_SEG_APPEND_FULL); a record
 * flagged RAMCRC_SEG_ENTRY_OVERLONG never fits.  Outputs of a source segment
 * without RAMCRC_SEG_OK stay empty (RAMCRC_SEG_SOURCE_BAD).
 *
 * d_out_certs[k] = {head, checksum} is Segment::getAppendedLength's
 * certificate (src/Segment.cc:672-684) of output k, computed from the
 * placement sizes in the same pass (the outputs are not read back; it equals
 * what ramcrc_segments_certify_device returns for them); d_out_status[k] =
 * {flags, entries appended}.  Bytes of an output at or past its head are
 * never written.
 *
 * The list (d_place, *d_n_place entries on the device, at most place_cap)
 * must not decrease in `record`; with the walk's table order every output
 * then receives its entries in source-offset order, as build appends them.
 * The call refuses -- none of d_out, d_out_certs, d_out_status is written and
 * ramcrc_ctx_check returns RAMCRC_EREFUSED -- when the list decreases, names
 * a record at or beyond min(*d_n_entries, entries_cap) or a partition >=
 * n_part, when *d_n_place > place_cap, or when the table's segments are not
 * contiguous runs.
 *
 * d_base 16-byte aligned, seg_stride a multiple of 16 (the walk's rules);
 * d_out and out_stride are free; n_part > 0; out_stride >= out_capacity;
 * place_cap < 2^32; the output range must not overlap the source range.
 * Scratch comes from the context: after ramcrc_ctx_reserve(ctx, 16 + 4 *
 * n_seg + (n_part > 512 ? 4 * n_seg * n_part : 0), place_cap / 2 + 1), or
 * after one call of the same shape, it does not allocate.  Stream-ordered,
 * asynchronous. */
int ramcrc_recovery_append_device(ramcrc_ctx* ctx, const void* d_base, uint64_t seg_stride,
                                  uint64_t n_seg, const ramcrc_seg_status* d_status,
                                  const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                  const uint64_t* d_n_entries, const ramcrc_placement* d_place,
                                  uint64_t place_cap, const uint64_t* d_n_place, uint32_t n_part,
                                  void* d_out, uint64_t out_stride, uint32_t out_capacity,
                                  ramcrc_seg_cert* d_out_certs, ramcrc_append_status* d_out_status,
                                  void* stream);

/* The same on the host, single-threaded, for a backup without a GPU: host
 * pointers, n_entries records in `entries`, n_place placements in `place`.
 * Returns RAMCRC_EINVAL where the device form refuses (nothing is written).
 * No alignment rules. */
int ramcrc_recovery_append_host(const void* base, uint64_t seg_stride, uint64_t n_seg,
                                const ramcrc_seg_status* status, const ramcrc_seg_entry* entries,
                                uint64_t n_entries, const ramcrc_placement* place, uint64_t n_place,
                                uint32_t n_part, void* out, uint64_t out_stride,
                                uint32_t out_capacity, ramcrc_seg_cert* out_certs,
                                ramcrc_append_status* out_status);

/* The placement decision of RecoverySegmentBuilder::build
 * (src/RecoverySegmentBuilder.cc:74-201): for every walked record the key hash
 * (Key::getHash, src/Key.cc:140-151: MurmurHash3 x64-128 of the key, seeded
 * with the low 32 bits of the table id, first output word), the tablet lookup
 * (whichPartition, :330-343) and the liveness test (isEntryAlive, :300-307).
 * It writes the {record, partition} list ramcrc_recovery_append_device takes,
 * so walk -> partition -> append builds sealed recovery segments from replicas
 * in device memory without a host round trip. */
#define RAMCRC_LOG_ENTRY_TYPE_SEGHEADER 1u   /* LOG_ENTRY_TYPE_SEGHEADER, src/LogEntryTypes.h:32 */
#define RAMCRC_LOG_ENTRY_TYPE_RPCRESULT 7u   /* LOG_ENTRY_TYPE_RPCRESULT, src/LogEntryTypes.h:50 */

typedef struct ramcrc_tablet {      /* one ProtoBuf::Tablets::Tablet of the RecoveryPartition */
    uint64_t table_id;
    uint64_t start_key_hash;        /* inclusive */
    uint64_t end_key_hash;          /* inclusive */
    uint64_t ctime_segment_id;      /* ctime_log_head_id */
    uint32_t ctime_offset;          /* ctime_log_head_offset */
    uint32_t partition;             /* user_data; must be < n_part */
} ramcrc_tablet;

typedef struct ramcrc_partition_status {   /* per source segment */
    uint32_t flags;      /* RAMCRC_SEG_OK | RAMCRC_SEG_SOURCE_BAD | RAMCRC_SEG_NO_HEADER | RAMCRC_SEG_MALFORMED */
    uint32_t placed;     /* placements emitted */
    uint32_t unplaced;   /* records with no tablet ("Couldn't place object") */
    uint32_t dead;       /* records dropped by isEntryAlive */
} ramcrc_partition_status;

#define RAMCRC_SEG_NO_HEADER 512u    /* a record build would place has no usable SEGHEADER before
                                        it (build DIEs there): the segment places nothing */
#define RAMCRC_SEG_MALFORMED 1024u   /* some record is too short for its type's fields (our
                                        rule, below); that record is not placed */

/* Source segment s (d_base + s * seg_stride) is handled in the order of its
 * records in the walk's table (d_status, d_entries, *d_n_entries: a walk's
 * outputs; min(*d_n_entries, entries_cap) records are read).  d_part_status[s]
 * is RAMCRC_SEG_OK plus RAMCRC_SEG_MALFORMED when it applies, or:
 *   RAMCRC_SEG_SOURCE_BAD  d_status[s] lacks RAMCRC_SEG_OK (RAMCRC_SEG_TABLE_FULL
 *                          included): build throws before its loop.  Nothing is
 *                          placed or counted, the records' hashes read 0;
 *   RAMCRC_SEG_NO_HEADER   a record of a placed type (below) has no SEGHEADER
 *                          record before it in the segment, or the latest one
 *                          before it is shorter than the 20 bytes that hold its
 *                          segmentId (or not readable: RAMCRC_SEG_ENTRY_OVERLONG, a
 *                          payload past seg_stride).  Nothing is placed, and
 *                          placed, unplaced and dead read 0 (MALFORMED may be
 *                          set beside it; the hashes are still written).
 * The log position of a record is {the u64 at payload byte 8 of the latest
 * SEGHEADER record before it in its segment (SegmentHeader::segmentId,
 * src/LogMetadata.h:51-61), the record's offset}.
 *
 * Per record, by type (offsets are payload-relative; other types -- SEGHEADER,
 * LOGDIGEST, TABLESTATS, INVALID, unknown ones -- place nothing):
 *   SAFEVERSION  one placement for each partition 0 .. n_part-1, ascending; no
 *                tablet lookup, no liveness test (:101-116);
 *   TXPLIST      count = u32 at 16, participants {tableId, keyHash, rpcId} of
 *                24 bytes each from byte 24 (src/ParticipantList.h:81-112): in
 *                participant order one placement per participant whose tablet
 *                is found (the same partition may repeat); no liveness test
 *                (:118-141);
 *   OBJ          tableId = u64 at 16, numKeys = u8 at 24, the first key's
 *                length = u16 at 25 (cumulativeLengths[0]), its bytes from
 *                25 + 2 * numKeys (src/Object.h:40-45,137-181); numKeys 0 or
 *                length 0 hashes the empty key;
 *   PREP         the same 32 bytes further on (src/PreparedOp.h:63-94);
 *   OBJTOMB      tableId = u64 at 0, key = [32, length) (src/Object.h:285-336);
 *   RPCRESULT, PREPTOMB, TXDECISION   tableId = u64 at 0, the stored keyHash =
 *                u64 at 8 (src/RpcResult.h:75-126, src/PreparedOp.h:142-182,
 *                src/TxDecisionRecord.h:62-138).
 * The last six place at most once: whichPartition picks the first tablet in
 * list order with table_id equal and start_key_hash <= hash <= end_key_hash
 * (unsigned; tablets may overlap); none found counts in `unplaced`.  Then the
 * record is alive when its position >= {ctime_segment_id, ctime_offset} of
 * that tablet (segment id first, then offset), else it counts in `dead`.  An
 * alive record gets one placement {record, tablet.partition}.
 *
 * Malformed records (the reference's behaviour there is undefined; this rule
 * is this library's): a record of a placed type that carries
 * RAMCRC_SEG_ENTRY_OVERLONG or whose payload runs past seg_stride; an OBJ / PREP
 * shorter than 25 / 57 bytes, or with numKeys > 0 and shorter than the u16 key
 * length or the end of the first key; an OBJTOMB shorter than 32 bytes; an
 * RPCRESULT, PREPTOMB or TXDECISION shorter than 16; a TXPLIST shorter than its
 * 24-byte header or than 24 + 24 * count.  Such a record is not placed, counts
 * nowhere, its hash reads 0, and its segment gets RAMCRC_SEG_MALFORMED.
 *
 * d_key_hash (nullable, one slot per record read) receives the computed or
 * stored hash of every OBJ, PREP, OBJTOMB, RPCRESULT, PREPTOMB and TXDECISION
 * record of a segment with RAMCRC_SEG_OK, and 0 for every other record.
 *
 * The list goes to d_place in record order (it does not decrease in `record`)
 * and its length to *d_n_place (device), as ramcrc_recovery_append_device
 * reads them.  When more than place_cap placements are needed, *d_n_place
 * still receives the needed count, only the first place_cap are written, and
 * this call does not refuse: the append does, by its own *d_n_place >
 * place_cap rule.  Slots of d_place at or past the list's end are not written.
 *
 * The call refuses -- *d_n_place = 0 is its only output, and ramcrc_ctx_check
 * returns RAMCRC_EREFUSED -- when n_part is 0, a tablet names a partition >=
 * n_part, a record a segment >= n_seg, or the table's segments are not
 * contiguous runs.
 *
 * d_base 16-byte aligned, seg_stride a multiple of 16 (the walk's rules);
 * n_seg, entries_cap, place_cap < 2^32.  Up to 256 tablets are staged in LDS;
 * longer lists are read from device memory in the same order.  Scratch comes
 * from the context: after ramcrc_ctx_reserve(ctx, 16 + 9 * n_seg,
 * entries_cap), or after one call of the same shape, it does not allocate.
 * Stream-ordered, asynchronous. */
int ramcrc_recovery_partition_device(ramcrc_ctx* ctx, const void* d_base, uint64_t seg_stride,
                                     uint64_t n_seg, const ramcrc_seg_status* d_status,
                                     const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                     const uint64_t* d_n_entries, const ramcrc_tablet* d_tablets,
                                     uint32_t n_tablets, uint32_t n_part,
                                     ramcrc_placement* d_place, uint64_t place_cap,
                                     uint64_t* d_n_place, uint64_t* d_key_hash,
                                     ramcrc_partition_status* d_part_status, void* stream);

/* The same on the host, single-threaded: host pointers, n_entries records,
 * *n_place receives the needed count (at most place_cap placements are
 * written).  Returns RAMCRC_EINVAL where the device form refuses (nothing is
 * written).  No alignment rules. */
int ramcrc_recovery_partition_host(const void* base, uint64_t seg_stride, uint64_t n_seg,
                                   const ramcrc_seg_status* status,
                                   const ramcrc_seg_entry* entries, uint64_t n_entries,
                                   const ramcrc_tablet* tablets, uint32_t n_tablets,
                                   uint32_t n_part, ramcrc_placement* place, uint64_t place_cap,
                                   uint64_t* n_place, uint64_t* key_hash,
                                   ramcrc_partition_status* part_status);

/* The decision ObjectManager::replaySegment makes after each checksum check
 * (src/ObjectManager.cc:671-734 for objects, :766-867 for tombstones): is this
 * object or tombstone the newest thing known for its key, or is it discarded?
 * A recovering partition's table starts empty, so the outcome is a function of
 * the batch alone, and this call computes it for every walked record at once.
 * It also writes the survivors as a {record, 0} list that
 * ramcrc_recovery_append_device takes unchanged with n_part = 1, so walk ->
 * verify -> resolve -> append compacts recovery segments into side-log-shaped
 * segments that hold only what the master keeps, without a host round trip.
 * The call decides; it inserts nothing (the master's hash table and log stay
 * the master's).
 *
 * Inputs are a walk's outputs over n_seg segments (d_status, d_entries,
 * *d_n_entries; min(*d_n_entries, entries_cap) records are read).
 *
 * Participants.  A record takes part when it is an OBJ or OBJTOMB record of a
 * segment whose status has RAMCRC_SEG_OK and is well-formed by the partition
 * call's rules above (fields, first key of a multi-key object, malformed
 * records).  Nothing else takes part: other types -- PREP included, whose
 * replay depends on the order of arrival (:966-989) --, records of segments
 * without RAMCRC_SEG_OK, and malformed OBJ / OBJTOMB records of OK segments,
 * which are counted in `malformed`.  A failed object checksum does not exclude
 * a record: the reference only logs it (:664-669).
 *
 * Key identity.  Two participants have the same key when they share the table
 * id (all 64 bits: OBJ u64 at payload 16, OBJTOMB u64 at 0), the key length,
 * and the key bytes (OBJ: the first key, as the partition call finds it;
 * OBJTOMB: [32, length)).  The empty key is a key.  The 64-bit key hash only
 * narrows the search; equal hashes never make two keys equal.
 *
 * Version.  OBJ: u64 at payload 8 (Object::Header::version, src/Object.h:171);
 * OBJTOMB: u64 at 16 (objectVersion, :324).  Compared unsigned, all 64 bits.
 *
 * Winner of a key, in order: the highest version; among those a tombstone
 * before an object (:693 discards an object at <=, :786 a tombstone only at
 * <); among those the lowest record index.  This is the content of the
 * reference's hash table after replaying the table's records in table order.
 * For any other order it is the same, except for which of several records of
 * identical version and type is kept.  The tie rule among equal tombstones is
 * this library's own: the reference asserts that the case does not occur
 * (:790-793).
 *
 * safe_version is the maximum, over the SAFEVERSION records of at least 12
 * bytes in OK segments (readable: no RAMCRC_SEG_ENTRY_OVERLONG, payload inside
 * seg_stride), of the u64 at payload 0 (:875, :901), or 0 when there is none.
 *
 * What the call does not do: PREP and the other transaction records
 * (RPCRESULT, PREPTOMB, TXDECISION, TXPLIST), which take no part; the
 * raiseSafeVersion(version + 1) of a kept tombstone at :797, which depends on
 * the replay order and is not folded into safe_version; the tombstones
 * sequential replay synthesizes for an object it overwrites (:697-717,
 * :804-835); and insertion into the master's table.  A surviving tombstone is
 * listed as it lies in its segment: the reference rewrites its segment id,
 * timestamp and checksum before it logs it (:845-851); that rewrite is
 * ramcrc_replay_sidelog_device's, which takes this call's live list. */
#define RAMCRC_RESOLVE_NONE 0xFFFFFFFFu
typedef struct ramcrc_resolve_counts {
    uint64_t objects, tombstones;            /* participants */
    uint64_t live_objects, live_tombstones;  /* winners (one per distinct key) */
    uint64_t malformed;                      /* malformed OBJ / OBJTOMB records of OK segments */
    uint64_t safe_version;
} ramcrc_resolve_counts;

/* d_key_hash (nullable, one per record read) is the partition call's
 * d_key_hash output for the same table; with NULL the call computes
 * Key::getHash itself.  A caller's hashes must be a function of (table id,
 * key): equal keys with different hashes are treated as different keys.
 *
 * d_winner (nullable, one slot per record read) receives for every
 * participant the record index of the winner of its key, and
 * RAMCRC_RESOLVE_NONE for every other record; record i is live exactly when
 * d_winner[i] == i.  d_live receives {record, 0} for every live record,
 * objects and tombstones alike, in increasing record order, and *d_n_live
 * (device) the needed count; past live_cap only the first live_cap entries are
 * written, slots at or past the list's end are never written, and this call
 * does not refuse: the append then does, by its own *d_n_place > place_cap
 * rule.  d_counts (device) receives the counters.
 *
 * The call refuses -- *d_n_live = 0 and zeroed *d_counts are its only outputs,
 * and ramcrc_ctx_check returns RAMCRC_EREFUSED -- when a record names a
 * segment >= n_seg.
 *
 * d_base 16-byte aligned, seg_stride a multiple of 16 (the walk's rules);
 * n_seg, entries_cap, live_cap < 2^32 - 1.  Records are grouped in an
 * open-addressed table of S(n) slots, S(n) the smallest power of two that is
 * at least 64 and at least 2 * n, sized on the device from the walked count.
 * Scratch comes from the context: after ramcrc_ctx_reserve(ctx, 16 + 6 *
 * S(entries_cap), 2 * entries_cap), or after one call of the same shape, it
 * does not allocate.  Stream-ordered, asynchronous. */
int ramcrc_replay_resolve_device(ramcrc_ctx* ctx, const void* d_base, uint64_t seg_stride,
                                 uint64_t n_seg, const ramcrc_seg_status* d_status,
                                 const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                 const uint64_t* d_n_entries, const uint64_t* d_key_hash,
                                 uint32_t* d_winner, ramcrc_placement* d_live, uint64_t live_cap,
                                 uint64_t* d_n_live, ramcrc_resolve_counts* d_counts, void* stream);

/* The same on the host, single-threaded: host pointers, n_entries records,
 * *n_live receives the needed count (at most live_cap entries are written).
 * Returns RAMCRC_EINVAL where the device form refuses (nothing is written).
 * No alignment rules. */
int ramcrc_replay_resolve_host(const void* base, uint64_t seg_stride, uint64_t n_seg,
                               const ramcrc_seg_status* status, const ramcrc_seg_entry* entries,
                               uint64_t n_entries, const uint64_t* key_hash, uint32_t* winner,
                               ramcrc_placement* live, uint64_t live_cap, uint64_t* n_live,
                               ramcrc_resolve_counts* counts);

/* The same decision fed batch by batch: a table that outlives a call.
 * MasterService::recover (src/MasterService.cc:3501-3720) replays recovery
 * segments as they arrive from the backups (:3632), so every lookup after the
 * first segment meets a table that is not empty (src/ObjectManager.cc:678-696,
 * :766-793).  A replay table takes one walk's records per add and gives, at
 * any time, the verdict on any added batch as the table stands: exactly
 * ramcrc_replay_resolve_device's over everything added so far.
 *
 * Reused rules.  Participants, key identity, version, safe_version and the
 * malformed count are ramcrc_replay_resolve_device's above (resolve_rules.h,
 * partition_rules.h).
 *
 * Record identity.  A record is named {batch, record}.  Batches are numbered
 * 0, 1, 2 ... in the order they are added; "none" is {0xFFFFFFFF, 0xFFFFFFFF}.
 *
 * Winner of a key, over all batches added so far, in order: the highest
 * version; then a tombstone before an object; then the lowest {batch,
 * record}, batch first.
 *
 * The defining property.  Let C be the concatenation of the added batches'
 * record tables in add order, with segment numbers offset by the earlier
 * batches' n_seg.  The winners are what ramcrc_replay_resolve_host returns
 * for C, with global index i mapped back to {batch, record}.  The order in
 * which batches are added changes only which of several records of identical
 * version and type is kept.
 *
 * Hashes.  d_key_hash, where given, must be a function of (table id, key),
 * the same function for every add into a table until it is reset; NULL means
 * Key::getHash, computed in the call.  Under that rule two participants are
 * the same key exactly when table id, key length and key bytes are equal, and
 * that is what the table compares: it does not reject by hash.
 *
 * Lifetime.  A batch's segment bytes, status array, record table, hashes and
 * work array stay allocated and unchanged until the table is reset or
 * destroyed: a later add reads an earlier claimant's key from its segment, as
 * the one-call does within a batch, and a live query reads the work array.
 *
 * Spoiling.  Two things spoil a table: a record that names a segment >= n_seg,
 * and an add after which the table holds more than key_cap keys or in which a
 * record found no slot.  The refusal word is then set and ramcrc_ctx_check
 * returns RAMCRC_EREFUSED.  Until the next reset every add is a no-op on the
 * device, and every live and stats call writes only *d_n_live = 0 and zeroed
 * structures (spoiled = 1); d_winner and d_live stay untouched.  The add that
 * spoils has changed the table before it finds out: a pre-pass that validated
 * a batch before touching the table would cost one more read of the record
 * table per add, and is not made.
 *
 * Not done, as in the one-call: the synthesized tombstone for an overwritten
 * object (:697-717, :804-835), raiseSafeVersion(version + 1) (:797), PREP and
 * the other transaction records, and insertion into the master's own table:
 * the table is one of its own, asked by batch with live and by key with
 * ramcrc_replay_table_lookup_device, below.  The rewrite of a kept
 * tombstone's header is ramcrc_replay_sidelog_device's, below.
 *
 * Concurrency.  All calls are stream-ordered and asynchronous; calls on one
 * table are serialised by the handle; a caller who uses several streams
 * orders them. */
typedef struct { uint32_t batch, record; } ramcrc_replay_ref;
typedef struct ramcrc_replay_table ramcrc_replay_table;
typedef struct ramcrc_replay_table_stats {
    uint64_t keys;                           /* claimed slots: distinct keys */
    uint64_t live_objects, live_tombstones;  /* winners over the whole table */
    uint64_t safe_version;
    uint64_t batches;                        /* added since the last reset */
    uint64_t spoiled;                        /* 1: every other field is 0 */
} ramcrc_replay_table_stats;
#define RAMCRC_REPLAY_TABLE_MAX_BATCHES 65536u

/* One device allocation is made here and none afterwards: 16 + 32 *
 * max_batches + 4 * S 64-bit words, S = S(key_cap) slots of four words (the
 * key's highest version, its pick, its claim, one spare, so that a slot never
 * straddles a 128-byte line), a descriptor and a line of counters per batch,
 * a head of counters with the refusal word.  1 <= max_batches <= 65,536, so
 * that a rank (is_object << 48 | batch << 32 | record) fits one word; key_cap
 * < 2^32 - 1.  The table belongs to ctx and must be destroyed before it. */
int ramcrc_replay_table_create(ramcrc_ctx* ctx, uint64_t key_cap, uint32_t max_batches,
                               ramcrc_replay_table** out);
int ramcrc_replay_table_destroy(ramcrc_replay_table* t);

/* Empties the table and forgets its batches (their arrays are the caller's
 * again once the stream reaches this point).  Stream-ordered, on the device. */
int ramcrc_replay_table_reset(ramcrc_replay_table* t, void* stream);

/* Resolves one walk's records (d_status, d_entries, *d_n_entries over n_seg
 * segments) into the table.  d_work: the caller's array of entries_cap 64-bit
 * words, opaque; the add writes it and the live query reads it.  *batch (host,
 * nullable) receives the batch's number, assigned on the host under the
 * handle's lock.  Pointer, alignment and range rules are the one-call's.  With
 * max_batches batches already added it returns RAMCRC_EINVAL and launches
 * nothing. */
int ramcrc_replay_table_add_device(ramcrc_replay_table* t, const void* d_base, uint64_t seg_stride,
                                   uint64_t n_seg, const ramcrc_seg_status* d_status,
                                   const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                   const uint64_t* d_n_entries, const uint64_t* d_key_hash,
                                   uint64_t* d_work, uint32_t* batch, void* stream);

/* The verdict on one added batch's records as the table stands now; it may be
 * asked at any time and again after later adds.  d_winner[i] (nullable, one
 * per record read) is the winner of record i's key, or none.  d_live and
 * *d_n_live list the batch's records that are winners now, as {record, 0} in
 * increasing record order: ramcrc_recovery_append_device takes that list
 * unchanged with n_part = 1, over that batch's segments.  Past live_cap the
 * one-call's rule holds.  d_counts: objects, tombstones and malformed are the
 * batch's participants, noted at add time; live_* are the batch's winners
 * now; safe_version is the table's so far.  RAMCRC_EINVAL for a batch that
 * has not been added.  The tile sums come from the context's scratch: after
 * ramcrc_ctx_reserve(ctx, 0, entries_cap) the call does not allocate. */
int ramcrc_replay_table_live_device(ramcrc_replay_table* t, uint32_t batch,
                                    ramcrc_replay_ref* d_winner, ramcrc_placement* d_live,
                                    uint64_t live_cap, uint64_t* d_n_live,
                                    ramcrc_resolve_counts* d_counts, void* stream);

/* The whole table: one pass over the slots into *d_stats (device). */
int ramcrc_replay_table_stats_device(ramcrc_replay_table* t, ramcrc_replay_table_stats* d_stats,
                                     void* stream);

/* The same on the host, single-threaded: host pointers, n_entries records, no
 * alignment rules, the same lifetime rule.  ramcrc_replay_table_add_host
 * returns RAMCRC_EINVAL where the device form spoils, and the table is then
 * spoiled the same way: until the reset every add returns RAMCRC_EINVAL and
 * does nothing, and live and stats write *n_live = 0 and zeroed structures
 * (spoiled = 1) and return RAMCRC_OK. */
typedef struct ramcrc_replay_table_host ramcrc_replay_table_host;
int ramcrc_replay_table_create_host(uint64_t key_cap, uint32_t max_batches,
                                    ramcrc_replay_table_host** out);
int ramcrc_replay_table_destroy_host(ramcrc_replay_table_host* t);
int ramcrc_replay_table_reset_host(ramcrc_replay_table_host* t);
int ramcrc_replay_table_add_host(ramcrc_replay_table_host* t, const void* base, uint64_t seg_stride,
                                 uint64_t n_seg, const ramcrc_seg_status* status,
                                 const ramcrc_seg_entry* entries, uint64_t n_entries,
                                 const uint64_t* key_hash, uint64_t* work, uint32_t* batch);
int ramcrc_replay_table_live_host(ramcrc_replay_table_host* t, uint32_t batch,
                                  ramcrc_replay_ref* winner, ramcrc_placement* live,
                                  uint64_t live_cap, uint64_t* n_live,
                                  ramcrc_resolve_counts* counts);
int ramcrc_replay_table_stats_host(ramcrc_replay_table_host* t, ramcrc_replay_table_stats* stats);

/* What the table holds for a key: the batched form of ObjectManager::lookup
 * (src/ObjectManager.cc:2704-2741) and readObject (:325-369) as
 * MasterService::multiRead runs them per key (src/MasterService.cc:1352-1415),
 * against the replay table.  The live query answers by batch and record; this
 * call answers by key.  It reads the table and writes only its outputs.
 *
 * Answer.  Query q's answer is the winner, as the table stands now -- after
 * every add enqueued before the call on the stream and before any enqueued
 * after it --, of the key {table_id, key_len, the key_len bytes at d_keys +
 * key_off}.  Key identity is the table's: all 64 bits of the table id, the
 * length, the bytes; a hash only narrows the search.  The defining property:
 * for every participant record i of every added batch, the lookup of i's own
 * key returns as `ref` exactly what ramcrc_replay_table_live_device writes to
 * d_winner[i] for that batch at the same moment.  A key no participant
 * carries is RAMCRC_LOOKUP_ABSENT.
 *
 * Hashes.  d_key_hash[q], where given, must be the same function of (table
 * id, key) that the adds used; NULL means Key::getHash, computed in the call.
 *
 * Version and kind.  `version` is the winner's (OBJ: u64 at payload 8,
 * OBJTOMB: at 16); `kind` says which of the two it is.  A tombstone is what
 * readObject answers with STATUS_OBJECT_DOESNT_EXIST (:341); RejectRules are
 * the caller's, applied to the returned version.
 *
 * Value location (OBJECT only), after Object::getValueOffset / getValueLength
 * (src/Object.cc:647-676).  With nk = u8 at payload 24 the value begins at
 * payload offset 25 + 2 * nk + cum[nk - 1] (25 when nk = 0), cum[nk - 1] the
 * last u16 of the cumulative key length array.  value_off is that offset plus
 * the payload's offset in its segment, `segment` the winner's segment number
 * within its batch, value_len the rest of the payload: the value is the
 * value_len bytes at that batch's d_base + segment * seg_stride + value_off.
 * If the key table or the keys run past the payload -- only a multi-key
 * object can, since a participant's first key was checked -- value_len = 0
 * and value_off is the payload's end (the reference's getValueLength() == 0
 * when fillKeyOffsets fails).  Nothing outside the record's payload is read.
 *
 * Bad queries.  A query is RAMCRC_LOOKUP_BAD_KEY when key_len > 65,535,
 * reserved != 0, or key_off + key_len > keys_bytes (the sum in 64 bits,
 * overflow included).  Its ref is none and every other field is as for
 * ABSENT; no byte of the key buffer or the table is read for it; it neither
 * refuses the call nor sets the context's sticky bit.  Queries may repeat:
 * every copy gets the same answer.
 *
 * d_counts (nullable) receives how many queries got each kind; spoiled is 0.
 * On a spoiled table d_results stays untouched, *d_counts becomes {0, 0, 0,
 * 0, 1} and no new refusal is raised: the rule of live and stats.
 *
 * n_queries = 0 is legal (zeroed counts, nothing else); n_queries < 2^32 - 1;
 * d_queries 8-byte aligned, d_results 16-byte aligned, d_keys free.  Key
 * bytes are fetched as the aligned 16-byte words that hold at least one byte
 * of a usable query's key.  No table word, descriptor, work array or batch
 * counter is written: a lookup between two adds changes no later answer.
 * Lifetime and concurrency are the table's; the key buffer, queries and
 * hashes belong to the caller again once the stream has passed the call.
 * The counters use one 128-byte line of the context's scratch: after
 * ramcrc_ctx_reserve(ctx, 32, 0), or after any earlier call on the context
 * that reserved as much, a lookup does not allocate. */
typedef struct ramcrc_lookup_key {
    uint64_t table_id;   /* all 64 bits compared */
    uint64_t key_off;    /* byte offset of the key in the caller's key buffer */
    uint32_t key_len;    /* 0 .. 65,535 (KeyLength is 16 bits); the empty key is a key */
    uint32_t reserved;   /* must be 0 */
} ramcrc_lookup_key;     /* 24 bytes */

#define RAMCRC_LOOKUP_ABSENT    0u   /* no record of this key was ever added */
#define RAMCRC_LOOKUP_OBJECT    1u
#define RAMCRC_LOOKUP_TOMBSTONE 2u   /* readObject: STATUS_OBJECT_DOESNT_EXIST (:341) */
#define RAMCRC_LOOKUP_BAD_KEY   3u   /* the query itself is unusable; nothing was read for it */

typedef struct ramcrc_lookup_result {
    ramcrc_replay_ref ref;   /* the key's winner, {batch, record}; none = {0xFFFFFFFF, 0xFFFFFFFF} */
    uint64_t version;        /* the winner's version; 0 when there is none */
    uint32_t kind;           /* RAMCRC_LOOKUP_* */
    uint32_t segment;        /* OBJECT: the winner's segment number within its batch; else 0xFFFFFFFF */
    uint32_t value_off;      /* OBJECT: offset of the value from the start of that segment; else 0 */
    uint32_t value_len;      /* OBJECT: Object::getValueLength(); else 0 */
} ramcrc_lookup_result;      /* 32 bytes */

typedef struct ramcrc_lookup_counts {
    uint64_t objects, tombstones, absent, bad, spoiled;
} ramcrc_lookup_counts;

int ramcrc_replay_table_lookup_device(ramcrc_replay_table* t, const void* d_keys, uint64_t keys_bytes,
                                      const ramcrc_lookup_key* d_queries, uint64_t n_queries,
                                      const uint64_t* d_key_hash /* nullable */,
                                      ramcrc_lookup_result* d_results,
                                      ramcrc_lookup_counts* d_counts /* nullable */, void* stream);

/* The same on the host, single-threaded: host pointers, no alignment rules,
 * the same answers.  Returns RAMCRC_OK on a spoiled table, with the outputs
 * described above. */
int ramcrc_replay_table_lookup_host(ramcrc_replay_table_host* t, const void* keys, uint64_t keys_bytes,
                                    const ramcrc_lookup_key* queries, uint64_t n_queries,
                                    const uint64_t* key_hash, ramcrc_lookup_result* results,
                                    ramcrc_lookup_counts* counts);

/* A multi-read's reply: the loop of MasterService::multiRead
 * (src/MasterService.cc:1352-1415) over ObjectManager::readObject
 * (src/ObjectManager.cc:324-369) and rejectOperation (:2893-2907), against the
 * replay table.  The call looks every key up, applies the query's RejectRules,
 * and packs MultiOp::Response::ReadPart headers and object data back to back
 * into d_reply until the reply would pass reply_cap.  Rules marked "ours"
 * cover what the reference leaves uninitialised or where the packed query
 * form differs from the wire's.
 *
 * Lookup.  Queries, the key buffer, hashes, key identity, the bad-query test
 * and the moment of the answer are exactly ramcrc_replay_table_lookup_device's.
 * d_results, when not NULL, receives bit for bit what that call would write.
 * The call reads the table and the added batches' segments and writes only
 * its outputs.
 *
 * Status per query, in this order.
 *   - Ours: a bad query (RAMCRC_LOOKUP_BAD_KEY, or d_rules[q].reserved != 0)
 *     gets STATUS_REQUEST_FORMAT_ERROR (9), version 0, length 0, and the call
 *     goes on with the next query.
 *   - ABSENT or TOMBSTONE: STATUS_OBJECT_DOESNT_EXIST (3), before any rule is
 *     looked at (:341-342).  Ours: version 0, length 0 (the reference leaves
 *     both unset).
 *   - OBJECT with version v: version = v, then rejectOperation(rules, v)
 *     verbatim: v == 0 (VERSION_NONEXISTENT) gives 3 if doesnt_exist, else
 *     OK; exists gives STATUS_OBJECT_EXISTS (4); version_le_given && v <=
 *     given_version gives STATUS_WRONG_VERSION (5); version_ne_given && v !=
 *     given_version gives 5; otherwise STATUS_OK (0).  A rule byte is set when
 *     it is not 0.  A rejected object keeps its version; ours: its length is 0.
 *   d_rules = NULL: no rule is set for any query.  STATUS_UNKNOWN_TABLET is the
 *   tablet manager's: the caller applies it before the call.
 *
 * Part.  A part is MultiOp::Response::ReadPart (src/WireFormat.h:1140-1155),
 * packed, 16 bytes little-endian: {u32 status, u64 version, u32 length}.  Only
 * a STATUS_OK part is followed by `length` data bytes: by default the winner's
 * payload [24, payload length) -- key count, cumulative key lengths, keys and
 * value, as appendKeysAndValueToBuffer writes them (src/Object.cc:279-291) --,
 * with RAMCRC_READ_VALUE_ONLY the value_len bytes at value_off (possibly
 * none).  An object whose keys run past its payload has value_len 0 and still
 * sends its payload from 24 by default.  Parts lie back to back in query
 * order from d_reply + 0, so a part may start at any byte.  d_part_off[q]
 * (nullable) is the offset of query q's part, or RAMCRC_READ_NONE if q was not
 * returned.
 *
 * Truncation (:1364-1375).  With end_q the offset just past part q, the
 * returned queries are the leading ones with end_q <= reply_cap; `returned`
 * is their number (respHdr->count) and reply_bytes the last such end_q (0 when
 * none).  reply_cap is the caller's maxResponseRpcLen minus the 8-byte
 * MultiOp::Response header it writes itself; the reference's own test
 * (src/MasterServiceTest.cc:1450-1484) returns exactly one 1-byte-key,
 * 50-byte-value object at limit 78 = 8 + 16 + 54.  No byte of d_reply at or
 * past reply_bytes is written.  Ours: the summary's counters cover returned
 * parts only.  value_bytes and key_bytes are PerfStats' readObjectBytes
 * (getValueLength) and readKeyBytes (getKeysAndValueLength - getValueLength)
 * of the returned OK parts, in either mode.
 *
 * Queries may repeat: every copy gets its own part and its own data.
 * n_queries = 0 writes a zeroed summary and nothing else.  On a spoiled table
 * d_reply, d_part_off and d_results stay untouched, the summary is all zero
 * with spoiled = 1, and no new refusal is raised: the lookup's rule.
 *
 * RAMCRC_EINVAL before any launch: unknown flag bits; d_summary or d_queries
 * NULL with n_queries > 0; d_reply NULL with
 * reply_cap > 0; misaligned d_queries (8), d_rules (8), d_results (16),
 * d_part_off (8) or d_summary (8); n_queries >= 2^32 - 1.  d_reply and d_keys
 * need no alignment.  d_reply must not overlap any added batch's segments,
 * the key buffer or another argument; the call cannot check this.  Data
 * bytes are fetched as the aligned 16-byte words that hold at least one of
 * them.
 *
 * Scratch comes from the context: 32 + 8 * ceil(n_queries / 256) words and 4 *
 * n_queries entries.  After ramcrc_ctx_reserve(ctx, 32 + 8 * ceil(n / 256),
 * 4 * n), or after any earlier call on the context that reserved as much, a
 * read of up to n queries does not allocate.  The call is stream-ordered and
 * asynchronous; lifetime and concurrency are the table's. */
typedef struct ramcrc_reject_rules {   /* RejectRules, src/RejectRules.h:41-47, padded to 16 bytes */
    uint64_t given_version;
    uint8_t  doesnt_exist, exists, version_le_given, version_ne_given;
    uint32_t reserved;                 /* must be 0 */
} ramcrc_reject_rules;

#define RAMCRC_READ_VALUE_ONLY 1u      /* readObject's valueOnly; default: keys and value, as multiRead sends */
#define RAMCRC_READ_NONE 0xFFFFFFFFFFFFFFFFull

#define RAMCRC_STATUS_OK 0u                     /* src/Status.h */
#define RAMCRC_STATUS_OBJECT_DOESNT_EXIST 3u
#define RAMCRC_STATUS_OBJECT_EXISTS 4u
#define RAMCRC_STATUS_WRONG_VERSION 5u
#define RAMCRC_STATUS_REQUEST_FORMAT_ERROR 9u

typedef struct ramcrc_read_summary {
    uint64_t returned;        /* respHdr->count: leading queries whose part is in the reply */
    uint64_t reply_bytes;     /* end of the last returned part */
    uint64_t ok, doesnt_exist, object_exists, wrong_version, bad;  /* returned parts by status */
    uint64_t value_bytes;     /* PerfStats readObjectBytes of the returned OK parts */
    uint64_t key_bytes;       /* readKeyBytes: keysAndValueLength - valueLength, same parts */
    uint64_t spoiled;
} ramcrc_read_summary;

int ramcrc_replay_table_read_device(ramcrc_replay_table* t, const void* d_keys, uint64_t keys_bytes,
                                    const ramcrc_lookup_key* d_queries, uint64_t n_queries,
                                    const uint64_t* d_key_hash /* nullable */,
                                    const ramcrc_reject_rules* d_rules /* nullable: no rules */,
                                    uint32_t flags, void* d_reply, uint64_t reply_cap,
                                    uint64_t* d_part_off /* nullable, one per query */,
                                    ramcrc_lookup_result* d_results /* nullable */,
                                    ramcrc_read_summary* d_summary, void* stream);

/* The same on the host, single-threaded: host pointers, no alignment rules,
 * the same bytes.  Returns RAMCRC_OK on a spoiled table, with the outputs
 * described above. */
int ramcrc_replay_table_read_host(ramcrc_replay_table_host* t, const void* keys, uint64_t keys_bytes,
                                  const ramcrc_lookup_key* queries, uint64_t n_queries,
                                  const uint64_t* key_hash, const ramcrc_reject_rules* rules,
                                  uint32_t flags, void* reply, uint64_t reply_cap,
                                  uint64_t* part_off, ramcrc_lookup_result* results,
                                  ramcrc_read_summary* summary);

/* An indexed read's reply: the loop of MasterService::readHashes
 * (src/MasterService.cc:797-809) over ObjectManager::readHashes
 * (src/ObjectManager.cc:179-265), against the replay table.  IndexLookup gets
 * primary-key hashes from an indexlet and sends READ_HASHES to the master; the
 * call answers it: for every asked 64-bit hash, every object whose primary-key
 * hash equals it, packed back to back into d_reply.  No key is given and none
 * is compared.  Rules marked "ours" cover what the reference leaves open or
 * where this form differs from it.
 *
 * A record's hash is d_key_hash[record] of its batch when that batch was added
 * with hashes, and Key::getHash of its key, computed in the call, otherwise
 * (the survivor batch of a clean has none).  The asked hashes must be the
 * same function of (table id, key) that the adds used.  A table whose adds
 * were given anything but Key::getHash must not have been cleaned when this
 * call is made: otherwise which of the moved keys are found is unspecified.
 * Nothing wrong is ever returned: every object sent has a record hash equal to
 * the asked hash.  In the reference the asked value is Object::getPKHash(),
 * Key::getHash of key 0; the table's key already is an object's first key.
 *
 * Match.  For asked hash h the call walks the slots from h & (slots - 1) to
 * the first unclaimed one, at most every slot once: slots are never
 * un-claimed, so every key of h lies there.  A claimed slot matches when its
 * claimant's table id equals table_id -- ours: all 64 bits; the reference
 * compares only the hash (:241), and Key::getHash is seeded with the low 32
 * bits of the id -- and its claimant's record hash equals h.  A matching
 * slot's winner is the key's, exactly as the lookup names it: a tombstone
 * sends nothing (:235) and counts in `tombstones`, an object sends one part.
 *
 * Part.  12 bytes little-endian, {u64 version, u32 length} (:243-245), then
 * `length` bytes: the winner's payload [24, payload length), as
 * appendKeysAndValueToBuffer writes it; an object whose keys run past its
 * payload still sends its payload from byte 24, as the read does.  Parts lie
 * back to back from d_reply + 0 in the order of the asked hashes, so a part
 * may begin at any byte.  Ours: the objects of one hash go in ascending winner
 * {batch, record}, batch first (the reference's order is its bucket order;
 * slot order here depends on which lane won a claim inside an add and must
 * not show).  On the device a hash with one object is copied by the
 * workgroup; a hash with several is served by one lane, a chain walk per
 * object and its bytes one by one: right for the rare equal 64-bit hashes,
 * slow for a caller's own hash function that puts many or large objects under
 * one hash.  A hash may repeat in the request: every copy sends its objects
 * again.  d_parts[q] (nullable) is where hash q's first part begins and how
 * many objects it sent; a returned hash without an object has its offset and
 * objects = 0, a hash that was not returned {RAMCRC_READ_NONE, 0, 0}.
 *
 * Truncation (:258-263).  With start_q the offset at which hash q's parts
 * begin and end_q the offset just past them, the reference keeps hash q
 * exactly when start_q <= maxLength: it tests the length before the hash, so
 * the reply may pass maxLength by one hash's parts.  The returned hashes are
 * the leading ones with start_q <= max_length and, ours, end_q <=
 * reply_capacity, since a reply buffer here does not grow; with
 * reply_capacity >= max_length + the longest hash's parts the reference's
 * rule alone decides.  max_length is the caller's maxResponseRpcLen -
 * sizeof(ReadHashes::Response).  `hashes` is the number of returned hashes
 * (respHdr->numHashes), reply_bytes the last returned end_q, `objects` what is
 * in the reply.  objects_counted is `objects` plus the objects of the first
 * hash not returned, if there is one: what the reference leaves in
 * respHdr->numObjects, since :242 is not undone at :260; a caller sends the
 * honest figure, `objects`.  All other counters cover returned hashes only.
 * No byte of d_reply at or past reply_bytes is written.
 *
 * The tablet test of :218-226 (not owned, or locked for migration) is the
 * caller's: it cuts the request before the first hash it does not own.
 *
 * n_hashes = 0 writes a zeroed summary and nothing else.  On a spoiled table
 * d_reply and d_parts stay untouched, the summary is all zero with spoiled =
 * 1, and no new refusal is raised: the lookup's rule.  No table word,
 * descriptor, work array or batch counter is written: a call between two adds
 * changes no later answer.
 *
 * RAMCRC_EINVAL before any launch: flags != 0; d_summary NULL; d_hashes NULL
 * with n_hashes > 0; d_reply NULL with reply_capacity > 0; misaligned
 * d_hashes, d_parts or d_summary (8); n_hashes >= 2^32 - 1.  d_reply needs no
 * alignment and must not overlap any added batch's segments or another
 * argument; the call cannot check this.  Data bytes are fetched as the
 * aligned 16-byte words that hold at least one of them.
 *
 * Scratch comes from the context: 32 + 16 * ceil(n_hashes / 256) words and 6 *
 * n_hashes entries.  After ramcrc_ctx_reserve(ctx, 32 + 16 * ceil(n / 256),
 * 6 * n), or after any earlier call on the context that reserved as much, a
 * call of up to n hashes does not allocate.  The call is stream-ordered,
 * asynchronous and capturable and makes no host sync; lifetime and
 * concurrency are the table's. */
typedef struct ramcrc_hash_part {      /* one per asked hash; 16 bytes */
    uint64_t off;                      /* where the hash's first object part begins in the reply;
                                          RAMCRC_READ_NONE if the hash was not returned */
    uint32_t objects;                  /* objects sent for this hash (0 is a returned, empty hash) */
    uint32_t reserved;                 /* written as 0 */
} ramcrc_hash_part;

typedef struct ramcrc_read_hashes_summary {
    uint64_t hashes;           /* respHdr->numHashes: the leading hashes answered */
    uint64_t objects;          /* objects that are in the reply */
    uint64_t objects_counted;  /* respHdr->numObjects as the reference computes it, see Truncation */
    uint64_t reply_bytes;
    uint64_t value_bytes, key_bytes;   /* PerfStats readObjectBytes / readKeyBytes of the objects in the reply */
    uint64_t empty;            /* returned hashes with no object */
    uint64_t tombstones;       /* keys of returned hashes that matched and whose winner is a tombstone */
    uint64_t spoiled;
} ramcrc_read_hashes_summary;

int ramcrc_replay_table_read_hashes_device(ramcrc_replay_table* t, uint64_t table_id,
                                           const uint64_t* d_hashes, uint64_t n_hashes,
                                           uint32_t flags /* must be 0 */, void* d_reply,
                                           uint64_t reply_capacity, uint64_t max_length,
                                           ramcrc_hash_part* d_parts /* nullable */,
                                           ramcrc_read_hashes_summary* d_summary, void* stream);

/* The same on the host, single-threaded: host pointers, no alignment rules,
 * the same bytes.  Returns RAMCRC_OK on a spoiled table, with the outputs
 * described above. */
int ramcrc_replay_table_read_hashes_host(ramcrc_replay_table_host* t, uint64_t table_id,
                                         const uint64_t* hashes, uint64_t n_hashes, uint32_t flags,
                                         void* reply, uint64_t reply_capacity, uint64_t max_length,
                                         ramcrc_hash_part* parts, ramcrc_read_hashes_summary* summary);

/* One reply of a table enumeration: MasterService::enumerate
 * (src/MasterService.cc:409-456) over Enumeration::complete
 * (src/Enumeration.cc:269-351), against the replay table.  The call walks the
 * table's buckets from a cursor, selects the keys of one table id and tablet
 * hash range that no stale iterator frame hides, and packs {u32 length,
 * object} entries into d_payload until a byte limit or a bucket limit; the
 * summary carries the cursor to go on with.  No key and no hash is given: this
 * is the one call that walks the table instead of probing it.  Rules marked
 * "ours" cover what the reference leaves open or where this form differs.
 *
 * Buckets.  The table has S = slots buckets (summary.num_buckets); a key's
 * bucket is its home, hash & (S - 1), never the slot the key happens to lie
 * in.  This is HashTable::findBucketIndex (src/HashTable.cc:489-495) for S <
 * 2^48, which every table here is, so a frame written from this call's cursor
 * means the same to the reference's stale-frame filter.  The hash is the
 * record hash exactly as the read-hashes call defines it: d_key_hash[record]
 * of the claimant's batch when that was added with hashes, Key::getHash of the
 * claimant's key, computed in the call, otherwise; the same caveat for cleaned
 * tables applies.  The keys of bucket b lie on the chain from slot b to the
 * first unclaimed slot (slots are never un-claimed), which the call walks, at
 * most every slot once.  Slot order must not show: the payload is defined by
 * hashes and winners only.
 *
 * Selection (enumerateBucket, :58-108).  A claimed slot with record hash h is
 * selected when its claimant's table id equals table_id -- ours: all 64 bits
 * --, first_hash <= h <= last_hash, no stale frame hides it, and, for bucket
 * bucket_index only, h >= bucket_next_hash.  Stale frame f (any power-of-two
 * f.num_buckets, not necessarily S) hides h when f.tablet_start_hash <= h <=
 * f.tablet_end_hash and, with idx = (h & 0xffffffffffff) & (f.num_buckets -
 * 1), either idx < f.bucket_index or idx == f.bucket_index && h <
 * f.bucket_next_hash (:80-100).  A selected key whose winner is a tombstone
 * sends nothing (:67); one whose winner is an object sends one entry.  Ours:
 * the reference applies top().bucketNextHash to every later bucket as well
 * and never clears it (:103, :330), which loses keys after a bucket larger
 * than a whole reply; here it holds for the cursor's bucket alone and
 * next_hash is 0 once that bucket is finished.  The two agree unless one
 * bucket alone exceeds max_bytes.  first_hash > last_hash selects nothing.
 *
 * Entry (appendObjectsToBuffer, :128-154).  A u32 little-endian `length`, then
 * `length` bytes of the winner's payload from byte 0, header and checksum
 * included, as log.getEntry gives them.  With RAMCRC_ENUM_KEYS_ONLY `length`
 * is the offset of the value, so the entry ends before it; for an object
 * whose keys run past its payload that offset is the payload length.  Entries
 * lie back to back from d_payload + 0, so one may begin at any byte.
 *
 * Order.  Ascending bucket; within a bucket ascending {hash, winner batch,
 * winner record}.  Ours: the reference's order within a bucket is its cache
 * lines', except where it must cut a bucket, which it then sorts by hash
 * (:319-320); always sorting makes its two cases one.
 *
 * Cut.  lim = min(max_bytes, payload_capacity); max_bytes is the caller's
 * maxPayloadBytes less what the reply already holds.  A bucket is kept whole
 * when its last entry ends at or before lim (:145, :302-313).  The first
 * bucket that is not: when it is a later bucket of the call it is left out,
 * next_bucket names it and next_hash = 0; when it is bucket_index itself
 * (:318-332) its leading entries that end at or before lim are sent and
 * next_hash is the hash of the first entry not sent -- ours: the cut moves
 * back to before the first entry that has that hash, so a resume with h >=
 * next_hash sends nothing twice; if that leaves nothing, stuck = 1 (the
 * reference loops forever here) and the caller must offer more room.  Either
 * way full = 1.  With every bucket below the limit kept, next_bucket is that
 * limit, next_hash = 0 and full = 0.  Ours: bucket_limit (0: S).  The
 * reference scans until the reply is full or the table ends, a reply's worth
 * of work there and a pass over the rest of the table here; the caller bounds
 * the pass instead, and a reply cut short by bucket_limit is a legal
 * enumeration reply.  No byte at or past payload_bytes is written.  What to
 * do when next_bucket == num_buckets stays with the caller, with the
 * iterator's serialisation: pop frames, return tabletEndHash + 1 (:338-350).
 *
 * Summary.  objects, payload_bytes, value_bytes and key_bytes cover the
 * entries sent; value and key bytes are the objects' as the read counts them,
 * whatever the flags.  tombstones counts the selected keys of the buckets kept
 * whole whose winner is a tombstone.
 *
 * The call changes no table word, descriptor, work array or batch counter.  On
 * a spoiled table d_payload stays untouched and the summary is all zero with
 * spoiled = 1: the lookup's rule.
 *
 * RAMCRC_EINVAL before any launch: unknown flag bits; d_summary NULL or
 * misaligned (8); d_payload NULL with payload_capacity > 0; bucket_index > S;
 * bucket_limit not 0 and below bucket_index or above S; n_stale >
 * RAMCRC_ENUM_MAX_STALE; stale NULL with n_stale > 0; a stale frame whose
 * num_buckets is 0 or no power of two.  `stale` is host memory, read before
 * the call returns and carried in the launch descriptor.  d_payload needs no
 * alignment and must not overlap any added batch's segments; data bytes are
 * fetched as the aligned 16-byte words that hold at least one of them.
 *
 * Scratch comes from the context and grows with the buckets' tiles, not with
 * buckets or objects: 32 + 16 * ceil(n / 256) words for the n = bucket_limit -
 * bucket_index buckets of the call, no entries.  After ramcrc_ctx_reserve(ctx,
 * 32 + 16 * ceil(S / 256), 0), or after any earlier call on the context that
 * reserved as much, no call on the table allocates.  The price is a second
 * chain walk when the entries are copied.  The call is stream-ordered,
 * asynchronous and capturable and makes no host sync; lifetime and
 * concurrency are the table's. */
typedef struct ramcrc_enum_frame {      /* EnumerationIterator::Frame, 40 bytes */
    uint64_t tablet_start_hash, tablet_end_hash, num_buckets, bucket_index, bucket_next_hash;
} ramcrc_enum_frame;
#define RAMCRC_ENUM_KEYS_ONLY 1u
#define RAMCRC_ENUM_MAX_STALE 8u

typedef struct ramcrc_enumerate_summary {
    uint64_t num_buckets;      /* S, the table's slots: Frame::numBuckets of this table */
    uint64_t next_bucket;      /* Frame::bucketIndex to go on with */
    uint64_t next_hash;        /* Frame::bucketNextHash to go on with; 0 unless next_bucket was sent in part */
    uint64_t objects, payload_bytes;
    uint64_t value_bytes, key_bytes;   /* of the objects sent, counted as the read counts them */
    uint64_t tombstones;       /* selected keys of finished buckets whose winner is a tombstone */
    uint64_t full;             /* 1: a bucket below bucket_limit was cut or left out */
    uint64_t stuck;            /* 1: full, and nothing was sent: the first object alone does not fit */
    uint64_t spoiled;
} ramcrc_enumerate_summary;

int ramcrc_replay_table_enumerate_device(ramcrc_replay_table* t, uint64_t table_id,
        uint64_t first_hash, uint64_t last_hash,          /* requestedTabletStartHash, top().tabletEndHash */
        uint64_t bucket_index, uint64_t bucket_next_hash, /* the top frame's cursor */
        uint64_t bucket_limit,                            /* 0: S */
        const ramcrc_enum_frame* stale /* host */, uint32_t n_stale,
        uint32_t flags, void* d_payload, uint64_t payload_capacity, uint64_t max_bytes,
        ramcrc_enumerate_summary* d_summary, void* stream);

/* The same on the host, single-threaded: host pointers, no alignment rules,
 * the same bytes.  Returns RAMCRC_OK on a spoiled table, with the outputs
 * described above. */
int ramcrc_replay_table_enumerate_host(ramcrc_replay_table_host* t, uint64_t table_id,
        uint64_t first_hash, uint64_t last_hash, uint64_t bucket_index, uint64_t bucket_next_hash,
        uint64_t bucket_limit, const ramcrc_enum_frame* stale, uint32_t n_stale, uint32_t flags,
        void* payload, uint64_t payload_capacity, uint64_t max_bytes,
        ramcrc_enumerate_summary* summary);

/* A secondary index over the table, built and searched on the device: the
 * indexlet's half of an indexed read (IndexLookup: LOOKUP_INDEX_KEYS, then
 * READ_HASHES).  index_build extracts the {secondary key, primary-key hash}
 * entries of one table id and key index from the table's winners and sorts
 * them (IndexletManager::insertEntry, src/IndexletManager.cc:578-604, for
 * every key MasterService::requestInsertIndexEntries would send,
 * src/MasterService.cc:1993-2032); index_lookup is a batch of
 * IndexletManager::lookupIndexKeys (:611-709) over the sorted entries.  Its
 * hashes go to ramcrc_replay_table_read_hashes_device unchanged, on the same
 * stream, without a host round trip.  Rules marked "ours" cover what the
 * reference leaves open or where this form differs.
 *
 * Selection.  A claimed slot is selected when its key's winner now is an
 * OBJECT, its claimant's table id equals table_id -- ours: all 64 bits --, the
 * winner has more than index_id keys, its key table and keys lie within its
 * payload (the lookup's rule for a broken key table: such an object gets no
 * entry), a cumulative key length that shrinks or passes the last one gives no
 * entry either, and key index_id has length > 0.  Tombstone winners and
 * absent keys give no entry.  objects_seen counts the slots selected by table
 * id with an object winner, indexed or not.
 *
 * Entry.  {prefix, pk_hash, key_off, key_len, reserved = 0}, 32 bytes.  prefix
 * is the key's first 8 bytes as a big-endian integer, zero-padded on the
 * right.  pk_hash is the slot's record hash exactly as the read-hashes call
 * defines it (the hash the claimant's batch was added with, Key::getHash of
 * the claimant's key otherwise).  The key's bytes are copied to d_index_keys +
 * key_off: the index owns its keys and nothing in it points into an added
 * batch, so it stays valid, and merely stale, after later adds and after a
 * clean has handed the victims' segments back.  A stale entry is harmless as
 * in the reference: read_hashes and the client's isKeyInRange filter it.
 *
 * Order.  Ascending by key, then by pk_hash (key_less,
 * src/btreeRamCloud/Btree.h:1978-1985).  Keys compare as IndexKey::keyCompare
 * (src/IndexKey.cc:41-59) compares non-empty keys: memcmp over the common
 * length, bytes unsigned, then the shorter key first.  d_hashes[i] ==
 * d_entries[i].pk_hash for every i < n_entries, so a lookup's reply is a
 * contiguous copy.  Ours: entries equal in key and hash (two primary keys of
 * one 64-bit hash with the same secondary key; the tree would hold one) are
 * all kept, in unspecified relative order.  Ours: where a key lies in
 * d_index_keys is unspecified (slot order may show there and nowhere else);
 * the keys take key_bytes bytes from d_index_keys + 0, back to back.
 *
 * Summary and capacity.  entries_needed and key_bytes_needed are what the
 * selection comes to.  When entries_needed > entry_capacity or
 * key_bytes_needed > keys_capacity: overflow = 1, n_entries = key_bytes = 0
 * and no byte of d_entries, d_hashes and d_index_keys is written.  The call
 * with all three NULL and both capacities 0 is the sizing call.  Otherwise
 * n_entries = entries_needed, key_bytes = key_bytes_needed, and nothing at or
 * past them is written.  On a spoiled table the arrays stay untouched and the
 * summary is all zero with spoiled = 1.  The call changes no table word,
 * descriptor, work array or batch counter.
 *
 * RAMCRC_EINVAL before any launch: t or d_summary NULL; index_id == 0 (the
 * primary key is no index; an index_id above 255 selects nothing); d_entries or d_hashes NULL with
 * entry_capacity > 0; d_index_keys NULL with keys_capacity > 0;
 * entry_capacity >= 2^32 - 1; d_entries not 16-byte aligned, d_hashes or
 * d_summary not 8-byte aligned.  The outputs must not overlap any added
 * batch or each other; the call cannot check this.
 *
 * Scratch comes from the context: 32 + 16 * ceil(S / 256) words for the S
 * slots of the table, and, when entry_capacity exceeds one sort tile of 1,024
 * entries, 4 * entry_capacity entries for the merge passes' second buffer.
 * After ramcrc_ctx_reserve(ctx, 32 + 16 * ceil(S / 256), 4 * entry_capacity) a
 * build does not allocate.  The number of launches follows entry_capacity,
 * never the table's contents: the call is stream-ordered, asynchronous and
 * capturable and makes no host sync; lifetime and concurrency are the table's.
 *
 * Not done: insertEntry and removeEntry one at a time -- an index is rebuilt,
 * not edited --; the indexlet's boundaries (findIndexlet, firstNotOwnedKey,
 * STATUS_UNKNOWN_INDEXLET), the RPC header and the transport, which stay with
 * the master. */
typedef struct ramcrc_index_entry {      /* 32 bytes */
    uint64_t prefix;                     /* the key's first 8 bytes, big-endian, zero-padded */
    uint64_t pk_hash;                    /* the primary key's record hash */
    uint64_t key_off;                    /* the key's bytes: d_index_keys + key_off */
    uint32_t key_len;                    /* 1 .. 65,535 */
    uint32_t reserved;                   /* written as 0 */
} ramcrc_index_entry;

typedef struct ramcrc_index_build_summary {
    uint64_t n_entries, key_bytes;       /* what was written; 0 on overflow */
    uint64_t entries_needed, key_bytes_needed;
    uint64_t objects_seen;               /* object winners of table_id, indexed or not */
    uint64_t overflow;
    uint64_t spoiled;
} ramcrc_index_build_summary;

int ramcrc_replay_table_index_build_device(ramcrc_replay_table* t, uint64_t table_id, uint32_t index_id,
                                           ramcrc_index_entry* d_entries, uint64_t entry_capacity,
                                           uint64_t* d_hashes, void* d_index_keys, uint64_t keys_capacity,
                                           ramcrc_index_build_summary* d_summary, void* stream);

/* The same on the host table, single-threaded: host pointers, no alignment
 * rules, the same entries (std::stable_sort under the same comparator).  The
 * keys lie in d_index_keys in slot order of the host table, which may differ
 * from the device's: compare entries with key_off dereferenced. */
int ramcrc_replay_table_index_build_host(ramcrc_replay_table_host* t, uint64_t table_id, uint32_t index_id,
                                         ramcrc_index_entry* entries, uint64_t entry_capacity,
                                         uint64_t* hashes, void* index_keys, uint64_t keys_capacity,
                                         ramcrc_index_build_summary* summary);

/* A batch of IndexletManager::lookupIndexKeys (src/IndexletManager.cc:654-706)
 * over a built index.  The call takes a context, not a table: an index is
 * self-contained.  n_entries is read from d_build_summary on the device, so a
 * build and a lookup chain on one stream without a sync.
 *
 * Query.  {first_off, last_off, first_allowed_hash, first_len, last_len,
 * max_hashes, reserved = 0}, 40 bytes; the two keys lie at d_qkeys + first_off
 * and + last_off.  lo is the first entry not less than {first key,
 * first_allowed_hash} in the build's order (:654-662); hi is the first entry
 * whose key compares greater than the last key (:667).  The query returns num
 * = min(hi - lo, max_hashes) hashes, d_hashes[lo .. lo + num).  When hi - lo >
 * max_hashes it also returns the next entry to fetch (:686-690): next_entry =
 * lo + num, next_key_hash that entry's pk_hash, next_key_off and next_key_len
 * its key in d_index_keys; otherwise the four are 0.  An empty last key is
 * unbounded above, as keyCompare's keyLength2 == 0 rule makes it at :667.
 * Ours: an empty first key is below every entry.  The reference's comparator
 * is no consistent order for an empty first key -- keyCompare(x, empty) == -1
 * and keyCompare(empty, x) < 0 both hold --, and what its tree then returns is
 * an accident of the tree's shape.  A first key above the last key returns
 * nothing.  A query whose key ranges run past qkeys_bytes, a length > 65,535
 * or reserved != 0 is RAMCRC_INDEX_BAD_QUERY with no hashes; nothing is read
 * for it, as for the lookup's bad keys.
 *
 * Reply.  Queries are served in order and their hashes packed back to back in
 * d_out_hashes; out_off counts hashes.  The first query whose hashes would
 * end past out_capacity, and every later one, is RAMCRC_INDEX_NOT_SERVED and
 * writes no hash.  A result that is BAD_QUERY or NOT_SERVED is {out_off =
 * RAMCRC_READ_NONE, status, every other field 0}.  Summary: served counts the
 * leading queries that were not NOT_SERVED, bad ones included; hashes what was
 * written; bad and maxed_out (hi - lo > max_hashes) cover the served ones;
 * n_entries is the index's.  overflow_index = 1 when the build summary says
 * overflow or spoiled: then every query is NOT_SERVED and the other fields
 * are 0.  No word of d_out_hashes at or past `hashes` is written.
 *
 * RAMCRC_EINVAL before any launch: ctx, d_build_summary or d_summary NULL;
 * n_queries >= 2^32 - 1; d_queries or d_results NULL with n_queries > 0;
 * d_qkeys NULL with qkeys_bytes > 0; d_out_hashes NULL with out_capacity > 0;
 * a structure or hash array not 8-byte aligned (d_entries: 16).  d_entries,
 * d_hashes and d_index_keys may be NULL only for an index of no entries.  The
 * three arrays must be a build's: the call trusts key_off and key_len.
 *
 * Scratch comes from the context: 32 + 16 * ceil(n_queries / 256) words and 2 *
 * n_queries entries; after ramcrc_ctx_reserve(ctx, 32 + 16 * ceil(n / 256), 2 *
 * n) a call of up to n queries does not allocate.  Stream-ordered,
 * asynchronous, capturable, no host sync. */
#define RAMCRC_INDEX_OK         0u
#define RAMCRC_INDEX_BAD_QUERY  1u
#define RAMCRC_INDEX_NOT_SERVED 2u

typedef struct ramcrc_index_query {      /* 40 bytes */
    uint64_t first_off, last_off;        /* the keys' places in d_qkeys */
    uint64_t first_allowed_hash;
    uint32_t first_len, last_len;        /* 0: unbounded below / above */
    uint32_t max_hashes;
    uint32_t reserved;                   /* must be 0 */
} ramcrc_index_query;

typedef struct ramcrc_index_result {     /* 48 bytes */
    uint64_t out_off;                    /* in hashes; RAMCRC_READ_NONE: no answer */
    uint64_t next_entry;
    uint64_t next_key_hash;
    uint64_t next_key_off;
    uint32_t num_hashes;
    uint32_t next_key_len;               /* 0: the range is exhausted */
    uint32_t status;
    uint32_t reserved;                   /* written as 0 */
} ramcrc_index_result;

typedef struct ramcrc_index_lookup_summary {
    uint64_t served, hashes, bad, maxed_out;
    uint64_t n_entries;
    uint64_t overflow_index;
} ramcrc_index_lookup_summary;

int ramcrc_index_lookup_device(ramcrc_ctx* ctx, const ramcrc_index_entry* d_entries, const uint64_t* d_hashes,
                               const void* d_index_keys, const ramcrc_index_build_summary* d_build_summary,
                               const void* d_qkeys, uint64_t qkeys_bytes, const ramcrc_index_query* d_queries,
                               uint64_t n_queries, uint64_t* d_out_hashes, uint64_t out_capacity,
                               ramcrc_index_result* d_results, ramcrc_index_lookup_summary* d_summary,
                               void* stream);

/* The same on the host, single-threaded: host pointers, no alignment rules,
 * the same bytes. */
int ramcrc_index_lookup_host(const ramcrc_index_entry* entries, const uint64_t* hashes, const void* index_keys,
                             const ramcrc_index_build_summary* build_summary, const void* qkeys,
                             uint64_t qkeys_bytes, const ramcrc_index_query* queries, uint64_t n_queries,
                             uint64_t* out_hashes, uint64_t out_capacity, ramcrc_index_result* results,
                             ramcrc_index_lookup_summary* summary);

/* A multi-write: the loop of MasterService::multiWrite
 * (src/MasterService.cc:1523-1601) over ObjectManager::writeObject
 * (src/ObjectManager.cc:1181-1350), against the replay table.  The call does
 * not change the table.  It produces one sealed log segment with the new
 * objects and the tombstones of the objects they replace; the caller walks
 * that segment (ramcrc_segments_walk_device with *d_out_cert) and adds it as
 * the next batch.  A new object has the old version plus one, so it wins; its
 * tombstone carries the old version, so it beats the old object.  Reads
 * between the write and the add see the old state.  Rules marked "ours" cover
 * what the batch form must decide and the reference does not.
 *
 * Requests.  d_data holds keysAndValue images as MultiOp::Request::WritePart
 * carries them (src/WireFormat.h:1102-1115): {u8 key count nk, nk x u16
 * cumulative key lengths, the keys, the value}, at any byte.  Request q names
 * data_len bytes at data_off and the table.  The host form is the definition:
 * one loop in request order.
 *
 *   1. Usable.  The first key is found as ramcrc_part::parse finds an OBJ
 *      record's with the 24-byte header in front of the data (nk = 0: the
 *      empty key).  A request is bad -- STATUS_REQUEST_FORMAT_ERROR (9),
 *      version 0 -- when reserved != 0, d_rules[q].reserved != 0, data_off +
 *      data_len > data_bytes (64 bits, overflow included), 24 + data_len does
 *      not fit 32 bits, data_len < 1, or nk > 0 and (data_len < 3 or 1 + 2 nk
 *      + cum[0] > data_len).  Nothing of the data buffer or the table is read
 *      for a request the first four tests reject.  So every written object is
 *      a participant of a later add, keyed as the request was.
 *   2. Duplicates (ours).  Among the usable requests of one call the one with
 *      the lowest index is the only one served for its key (the table's key
 *      identity: table id, length, bytes).  Every later one gets STATUS_RETRY
 *      (17), version 0, and writes nothing, whatever became of the first.
 *   3. Current version.  w is the key's winner as the lookup returns it now;
 *      cur = w.version if w is an object, else 0 (:1218-1232).
 *   4. rejectOperation(rules, cur) verbatim (ramcrc_replay_table_read_device);
 *      a rejected request gets that status with version cur (:1234-1241).
 *   5. Version (:1245-1246).  cur != 0: v = cur + 1.  cur == 0: with a =
 *      next_version + the number of earlier requests of this call that reached
 *      this step with cur == 0 (allocateVersion runs before the space check, so
 *      a request that then does not fit has consumed one), ours: v = w.version
 *      + 1 if w is a tombstone of version >= a, else v = a.  The table does not
 *      raiseSafeVersion; without this rule a stale next_version would silently
 *      lose the write.  uint64_t arithmetic.
 *   6. Entries, in request order, each as Segment::append writes it (header
 *      byte with the minimal number of length bytes, the length, the payload:
 *      ramcrc_recovery_append_device's rules).  The object: 24 + data_len
 *      bytes, [4, 8) the timestamp, [8, 16) v, [16, 24) the table id, then the
 *      data unchanged, [0, 4) the finalized CRC32C of [4, end)
 *      (Object::computeChecksum, src/Object.cc:770-819).  Directly behind it,
 *      only when cur != 0 (:1254-1261), the tombstone: 32 + key_len bytes
 *      (src/Object.cc:839-851): the table id, the segment id
 *      d_batch_segment_id[w.batch] + w.segment (0 when the array is NULL), cur,
 *      the timestamp, the checksum of [0, 28) followed by the key (:1042-1057),
 *      the request's first key.
 *   7. Space (:1263-1301).  A request's entries go in together or not at all.
 *      The first served request with head + its bytes > out_capacity gets
 *      STATUS_RETRY with version cur; ours: so does every later request that
 *      reached this step.  Bad, duplicate and rejected requests behind the cut
 *      keep their status.  No byte at or past the final head is written.  A
 *      written request gets STATUS_OK and version v.
 *
 * Outputs.  d_parts: n_reqs packed 12-byte MultiOp::Response::WritePart, {u32
 * status, u64 version} little-endian (src/WireFormat.h:1168-1177), the reply's
 * body.  d_refs (nullable): where the request's entry headers lie in d_out,
 * 0xFFFFFFFF for an entry that was not written.  d_old (nullable): bit for bit
 * what ramcrc_replay_table_lookup_device writes for the request's first key
 * (writeObject's removedObjBuffer, as a place); for a request that is not
 * usable, the BAD_KEY answer.  *d_out_cert: {head, checksum},
 * Segment::getAppendedLength's certificate of d_out, what
 * ramcrc_segments_certify_device returns for it.  d_out starts empty: head 0
 * and a fresh Crc32C.
 *
 * Summary.  Requests by outcome; tombstones; allocated (step 5's count);
 * next_version: the larger of the input plus allocated and one past the highest
 * version step 5's tombstone rule gave (to a request that fit or not);
 * out_bytes; value_bytes and key_bytes (PerfStats writeObjectBytes and
 * writeKeyBytes, :1315-1318) over the OK requests; object_bytes and
 * tombstone_bytes, payload bytes of the written entries (TableStats'
 * byteCount).  On a spoiled table only the summary is written, all zero with
 * spoiled = 1, and no new refusal is raised: the lookup's rule.  n_reqs = 0
 * writes a zeroed summary with next_version passed through and the certificate
 * of an empty segment.
 *
 * RAMCRC_EINVAL before any launch: t, d_out_cert or d_summary NULL; d_reqs or
 * d_parts NULL with n_reqs > 0; d_data NULL with data_bytes > 0; d_out NULL
 * with out_capacity > 0; next_version = 0; n_reqs >= 2^32 - 1; misaligned d_reqs
 * (8), d_key_hash (8), d_rules (8), d_batch_segment_id (8), d_out_cert (4),
 * d_parts (4), d_refs (8), d_old (16) or d_summary (8).  d_data and d_out need
 * no alignment.  d_out must not overlap any input; the call cannot check this.
 * Data bytes are fetched as the aligned 16-byte words that hold at least one
 * byte of a usable request.  The call reads the table and the added batches'
 * segments and writes only its outputs: no table word changes.  Requests whose
 * appended sizes add up past 2^64 are not supported.
 *
 * Scratch comes from the context: with s = the grouping table's slots (the
 * smallest power of two >= max(64, 2 n)), 32 + 12 * ceil(n / 256) words and 8 *
 * n + 2 * s entries.  After ramcrc_ctx_reserve(ctx, 32 + 12 * ceil(n / 256),
 * 8 * n + 2 * s), or after any earlier call on the context that reserved as
 * much, a write of up to n requests does not allocate.  The call is
 * stream-ordered and asynchronous; lifetime and concurrency are the table's.
 *
 * Not done here: multiRemove is ramcrc_replay_table_remove_device and
 * multiIncrement is ramcrc_replay_table_increment_device, both below (the
 * request's `reserved` word stays 0); several output segments per call and a
 * SEGHEADER entry; RpcResult records; index entries; STATUS_UNKNOWN_TABLET and
 * transaction locks (the caller answers those before the call, as for the
 * read); incrementWriteCount; any change to the table itself. */
typedef struct ramcrc_write_req {
    uint64_t table_id;
    uint64_t data_off;   /* byte offset of the keysAndValue image in the data buffer */
    uint32_t data_len;
    uint32_t reserved;   /* must be 0 */
} ramcrc_write_req;      /* 24 bytes */

typedef struct ramcrc_write_ref {
    uint32_t object_off;      /* offset of the object's entry header in d_out; 0xFFFFFFFF: not written */
    uint32_t tombstone_off;   /* of the tombstone's; 0xFFFFFFFF: none */
} ramcrc_write_ref;

#define RAMCRC_STATUS_RETRY 17u                 /* src/Status.h */

typedef struct ramcrc_write_summary {
    uint64_t ok, doesnt_exist, object_exists, wrong_version, bad, retry_duplicate, retry_full;
    uint64_t tombstones;       /* written */
    uint64_t allocated;        /* versions taken from next_version on */
    uint64_t next_version;     /* the caller's safeVersion after the call */
    uint64_t out_bytes;        /* the output's head */
    uint64_t value_bytes;      /* PerfStats writeObjectBytes of the OK requests */
    uint64_t key_bytes;        /* writeKeyBytes: keysAndValueLength - valueLength, same requests */
    uint64_t object_bytes;     /* payload bytes of the written objects */
    uint64_t tombstone_bytes;  /* and of the written tombstones */
    uint64_t spoiled;
} ramcrc_write_summary;

int ramcrc_replay_table_write_device(ramcrc_replay_table* t, const void* d_data, uint64_t data_bytes,
                                     const ramcrc_write_req* d_reqs, uint64_t n_reqs,
                                     const uint64_t* d_key_hash /* nullable */,
                                     const ramcrc_reject_rules* d_rules /* nullable: no rules */,
                                     uint64_t next_version, uint32_t timestamp,
                                     const uint64_t* d_batch_segment_id /* nullable */,
                                     void* d_out, uint32_t out_capacity, ramcrc_seg_cert* d_out_cert,
                                     void* d_parts, ramcrc_write_ref* d_refs /* nullable */,
                                     ramcrc_lookup_result* d_old /* nullable */,
                                     ramcrc_write_summary* d_summary, void* stream);

/* The same on the host, single-threaded: host pointers, no alignment rules,
 * the same bytes.  Returns RAMCRC_OK on a spoiled table, with the outputs
 * described above. */
int ramcrc_replay_table_write_host(ramcrc_replay_table_host* t, const void* data, uint64_t data_bytes,
                                   const ramcrc_write_req* reqs, uint64_t n_reqs,
                                   const uint64_t* key_hash, const ramcrc_reject_rules* rules,
                                   uint64_t next_version, uint32_t timestamp,
                                   const uint64_t* batch_segment_id, void* out, uint32_t out_capacity,
                                   ramcrc_seg_cert* out_cert, void* parts, ramcrc_write_ref* refs,
                                   ramcrc_lookup_result* old, ramcrc_write_summary* summary);

/* A multi-remove: the loop of MasterService::multiRemove
 * (src/MasterService.cc:1435-1505) over ObjectManager::removeObject
 * (src/ObjectManager.cc:405-491), against the replay table.  The call does not
 * change the table.  It produces one sealed log segment with the tombstones of
 * the objects it removes; the caller walks that segment
 * (ramcrc_segments_walk_device with *d_out_cert) and adds it as the next
 * batch.  A tombstone carries the version of the object it removes, and at the
 * add a tombstone beats an object of the same version, so it wins.  Reads
 * between the remove and the add see the old state; a later write over the
 * removed key takes its version from the write's tombstone rule.  Rules marked
 * "ours" cover what the batch form must decide and the reference does not.
 *
 * Requests.  Request q is a lookup query: the table and key_len key bytes at
 * d_keys + key_off, at any byte (ramcrc_replay_table_lookup_device; hashes,
 * key identity and the moment of the answer are that call's).  d_rules[q],
 * where given, are its RejectRules as the read takes them.  The host form is
 * the definition: one loop in request order.
 *
 *   1. Usable.  A request is bad -- STATUS_REQUEST_FORMAT_ERROR (9), version
 *      0 -- when the lookup would answer RAMCRC_LOOKUP_BAD_KEY for it (key_len
 *      > 65,535, reserved != 0, key_off + key_len > keys_bytes in 64 bits,
 *      overflow included) or d_rules[q].reserved != 0.  Nothing of the key
 *      buffer or the table is read for it.
 *   2. Duplicates (ours, the write's rule).  Among the usable requests of one
 *      call the one with the lowest index is the only one served for its key
 *      (the table's key identity: table id, length, bytes).  Every later one
 *      gets STATUS_RETRY (17), version 0, and writes nothing, whatever became
 *      of the first.
 *   3. Lookup.  w is the key's winner as the lookup returns it now.  Not found
 *      means w.kind != OBJECT: absent, or a tombstone (:430-436).  Then the
 *      status is rejectOperation(rules, VERSION_NONEXISTENT) (:437-441):
 *      STATUS_OBJECT_DOESNT_EXIST (3) if doesnt_exist is set, else STATUS_OK;
 *      version 0; nothing is written.
 *   4. Found.  cur = w.version, whatever its value: the reference tests the
 *      entry's type, so an object of version 0 is found.  The status is
 *      rejectOperation(rules, cur) verbatim (ramcrc_replay_table_read_device);
 *      a rejected request gets that status with version cur (:443-447).  With
 *      cur = 0 that is status 3, version 0, if doesnt_exist is set; otherwise
 *      the request goes on.
 *   5. The tombstone (:454-456), one entry as Segment::append writes it: type
 *      LOG_ENTRY_TYPE_OBJTOMB, the minimal number of length bytes, then 32 +
 *      key_len payload bytes (src/Object.cc:839-851): the table id, the
 *      segment id d_batch_segment_id[w.batch] + w.segment (0 when the array is
 *      NULL), cur, the timestamp, the CRC32C of [0, 28) followed by the key
 *      (:1042-1057), the key's bytes from d_keys.
 *   6. Space (:474-478).  Entries lie in request order.  The first request of
 *      step 5 with head + its bytes > out_capacity gets STATUS_RETRY with
 *      version cur (*outVersion is set before the append); ours: so does every
 *      later request that reached step 5.  Requests that never reached step 5
 *      keep their status, also behind the cut.  No byte at or past the final
 *      head is written.  A written request gets STATUS_OK and version cur.
 *   7. Safe version (:487).  next_version out is the larger of next_version in
 *      and 1 + the highest cur over the written requests.  uint64_t
 *      arithmetic: cur = 2^64 - 1 leaves it unchanged.
 *
 * Outputs.  d_parts: n_reqs packed 12-byte MultiOp::Response::RemovePart, {u32
 * status, u64 version} little-endian (src/WireFormat.h:1157-1166), the reply's
 * body.  d_refs (nullable): the offset of the request's entry header in d_out,
 * 0xFFFFFFFF when nothing was written for it.  d_old (nullable): bit for bit
 * what ramcrc_replay_table_lookup_device writes for the request's key
 * (removeObject's removedObjBuffer, as a place: what a master needs to remove
 * index entries); for a request that is not usable, the BAD_KEY answer.
 * *d_out_cert: {head, checksum}, Segment::getAppendedLength's certificate of
 * d_out, what ramcrc_segments_certify_device returns for it.  d_out starts
 * empty: head 0 and a fresh Crc32C.
 *
 * Summary.  Requests by outcome: removed (STATUS_OK with a tombstone), ok_absent
 * (STATUS_OK with nothing to remove), the three rejections, bad,
 * retry_duplicate, retry_full; next_version (step 7); out_bytes;
 * tombstone_bytes, the payload bytes of the written tombstones (TableStats'
 * byteCount).  On a spoiled table only the summary is written, all zero with
 * spoiled = 1, and no new refusal is raised: the lookup's rule.  n_reqs = 0
 * writes a zeroed summary with next_version passed through and the certificate
 * of an empty segment.
 *
 * RAMCRC_EINVAL before any launch: t, d_out_cert or d_summary NULL; d_reqs or
 * d_parts NULL with n_reqs > 0; d_keys NULL with keys_bytes > 0; d_out NULL
 * with out_capacity > 0; next_version = 0; n_reqs >= 2^32 - 1; misaligned d_reqs
 * (8), d_key_hash (8), d_rules (8), d_batch_segment_id (8), d_out_cert (4),
 * d_parts (4), d_refs (4), d_old (16) or d_summary (8).  d_keys and d_out need
 * no alignment.  d_out must not overlap any input; the call cannot check this.
 * Key bytes are fetched as the aligned 16-byte words that hold at least one
 * byte of a usable request's key.  The call reads the table and the added
 * batches' segments and writes only its outputs: no table word changes.
 *
 * Scratch comes from the context: with s = the grouping table's slots (the
 * smallest power of two >= max(64, 2 n)), 32 + 10 * ceil(n / 256) words and 5 *
 * n + s entries.  After ramcrc_ctx_reserve(ctx, 32 + 10 * ceil(n / 256),
 * 5 * n + s), or after any earlier call on the context that reserved as
 * much, a remove of up to n requests does not allocate.  The call is
 * stream-ordered and asynchronous; lifetime and concurrency are the table's.
 *
 * Not done (multiIncrement is ramcrc_replay_table_increment_device, below):
 * several output segments per call and a SEGHEADER
 * entry; RpcResult records; index entries (d_old says where the removed object
 * lies); STATUS_UNKNOWN_TABLET and transaction locks (the caller answers those
 * before the call, as for the read); any change to the table itself. */
typedef struct ramcrc_remove_summary {
    uint64_t removed;        /* STATUS_OK with a tombstone written */
    uint64_t ok_absent;      /* STATUS_OK, nothing to remove */
    uint64_t doesnt_exist, object_exists, wrong_version, bad, retry_duplicate, retry_full;
    uint64_t next_version;   /* the caller's safeVersion after the call */
    uint64_t out_bytes;      /* the output's head */
    uint64_t tombstone_bytes;/* payload bytes of the written tombstones (TableStats byteCount) */
    uint64_t spoiled;
} ramcrc_remove_summary;

int ramcrc_replay_table_remove_device(ramcrc_replay_table* t, const void* d_keys, uint64_t keys_bytes,
                                      const ramcrc_lookup_key* d_reqs, uint64_t n_reqs,
                                      const uint64_t* d_key_hash /* nullable */,
                                      const ramcrc_reject_rules* d_rules /* nullable: no rules */,
                                      uint64_t next_version, uint32_t timestamp,
                                      const uint64_t* d_batch_segment_id /* nullable */,
                                      void* d_out, uint32_t out_capacity, ramcrc_seg_cert* d_out_cert,
                                      void* d_parts, uint32_t* d_refs /* nullable */,
                                      ramcrc_lookup_result* d_old /* nullable */,
                                      ramcrc_remove_summary* d_summary, void* stream);

/* The same on the host, single-threaded: host pointers, no alignment rules,
 * the same bytes.  Returns RAMCRC_OK on a spoiled table, with the outputs
 * described above. */
int ramcrc_replay_table_remove_host(ramcrc_replay_table_host* t, const void* keys, uint64_t keys_bytes,
                                    const ramcrc_lookup_key* reqs, uint64_t n_reqs,
                                    const uint64_t* key_hash, const ramcrc_reject_rules* rules,
                                    uint64_t next_version, uint32_t timestamp,
                                    const uint64_t* batch_segment_id, void* out, uint32_t out_capacity,
                                    ramcrc_seg_cert* out_cert, void* parts, uint32_t* refs,
                                    ramcrc_lookup_result* old, ramcrc_remove_summary* summary);

/* A multi-increment: the loop of MasterService::multiIncrement
 * (src/MasterService.cc:1277-1330) over incrementObject (:678-790), against
 * the replay table.  The call does not change the table.  It reads each key's
 * 8-byte value out of the added segments, adds to it, and produces one sealed
 * log segment with the new objects and the tombstones of the objects they
 * replace, exactly as a multi-write of the new values would; the caller walks
 * that segment (ramcrc_segments_walk_device with *d_out_cert) and adds it as
 * the next batch.  Reads between the increment and the add see the old state.
 * Rules marked "ours" cover what the batch form must decide and the reference
 * does not.
 *
 * Requests.  Request q is a lookup query, as the remove's: the table and
 * key_len key bytes at d_keys + key_off, at any byte.  d_args[q] holds its two
 * summands; d_rules[q], where given, its RejectRules as the read takes them.
 * The host form is the definition: one loop in request order.
 *
 *   1. Usable: the remove's step 1.  A request is bad --
 *      STATUS_REQUEST_FORMAT_ERROR (9), version 0 -- when the lookup would
 *      answer RAMCRC_LOOKUP_BAD_KEY for it or d_rules[q].reserved != 0.
 *      Nothing of the key buffer or the table is read for it.
 *   2. Duplicates (ours, the write's and the remove's rule).  Among the usable
 *      requests of one call the one with the lowest index is the only one
 *      served for its key.  Every later one gets STATUS_RETRY (17), version 0,
 *      and writes nothing, whatever became of the first.  Chaining several
 *      increments of one key within a call is not done: the caller adds the
 *      output and calls again.
 *   3. Read (readObject, src/ObjectManager.cc:340-351).  w is the key's winner
 *      as the lookup returns it now.  w not an object (absent, or a tombstone):
 *      STATUS_OBJECT_DOESNT_EXIST (3), version 0, if doesnt_exist is set (:697,
 *      :707); otherwise the old value is eight zero bytes, cur = 0, and the
 *      request goes on to step 5 (:707-712): no other rule applies.  w an
 *      object: cur = w.version, whatever its value, and the status is
 *      rejectOperation(rules, cur) verbatim; ours: a rejected request gets that
 *      status with version cur (the reference leaves the part's version unset).
 *   4. Eight bytes (:716-722).  A found object whose value_len != 8 gets
 *      STATUS_INVALID_OBJECT (22), version cur, and nothing is written; ours:
 *      lengths below 8 too, which the reference dereferences before it tests
 *      them.  The old value is the 8 bytes at the lookup's {batch, segment,
 *      value_off}, at any byte alignment.
 *   5. The sum (:741-749), on the old value's bits.  If add_int64 != 0 it is
 *      added as a two's-complement 64-bit integer that wraps.  Then, if
 *      add_double != 0.0, the bits are taken as an IEEE binary64 and add_double
 *      is added: round to nearest even, subnormals kept.  The comparison means
 *      that -0.0 adds nothing and that a NaN does add.  Ours: every NaN result
 *      is stored as 0x7FF8000000000000, so that host and device agree bit for
 *      bit.
 *   6. The object (:752-756).  Its keysAndValue image is {u8 1, u16 key_len,
 *      the key, the 8 new bytes}, 11 + key_len bytes; secondary keys of the old
 *      object are dropped, as in the reference.  From here on the request is
 *      steps 5-7 of ramcrc_replay_table_write_device with this image and cur
 *      (0 unless w is an object): the version with its allocation rank and
 *      tombstone rule, the object entry with its checksum, the old object's
 *      tombstone behind it only when cur != 0, the space check and the cut with
 *      STATUS_RETRY.  The updateRejectRules of :757-758 can never fire in a
 *      batch: nothing changes the table between the read and the write.
 *   7. The part.  d_parts: n_reqs packed 20-byte
 *      MultiOp::Response::IncrementPart, {u32 status, u64 version, u64 new
 *      value} little-endian (src/WireFormat.h:1124-1138).  A STATUS_OK part
 *      holds the new value's bits; every other part holds the bits of the
 *      request's add_double there, which :1319-1320 assign last.
 *
 * Outputs.  d_refs, d_old, *d_out_cert and d_out are the write's: where the
 * entry headers lie, the lookup's answer for the key (BAD_KEY for a request
 * that is not usable), Segment::getAppendedLength's certificate, an output that
 * starts empty.
 *
 * Summary.  Requests by outcome: ok, of which created (STATUS_OK without a
 * tombstone), the three rejections, invalid_object, bad, retry_duplicate,
 * retry_full; tombstones; allocated; next_version (the write's rule);
 * out_bytes; object_bytes and tombstone_bytes, payload bytes of the written
 * entries; value_bytes (8 per OK request) and key_bytes (3 + key_len each).  On
 * a spoiled table only the summary is written, all zero with spoiled = 1.
 * n_reqs = 0 writes a zeroed summary with next_version passed through and the
 * certificate of an empty segment.
 *
 * RAMCRC_EINVAL before any launch: t, d_out_cert or d_summary NULL; d_reqs,
 * d_args or d_parts NULL with n_reqs > 0; d_keys NULL with keys_bytes > 0;
 * d_out NULL with out_capacity > 0; next_version = 0; n_reqs >= 2^32 - 1;
 * misaligned d_reqs (8), d_args (8), d_key_hash (8), d_rules (8),
 * d_batch_segment_id (8), d_out_cert (4), d_parts (4), d_refs (8), d_old (16)
 * or d_summary (8).  d_keys and d_out need no alignment.  d_out must not
 * overlap any input; the call cannot check this.  Key bytes are fetched as the
 * aligned 16-byte words that hold at least one byte of a usable request's key,
 * the old value as the one or two aligned 16-byte words that hold it, inside
 * its segment.  The call reads the table and the added batches' segments and
 * writes only its outputs: no table word changes.
 *
 * Scratch comes from the context: with s = the grouping table's slots (the
 * smallest power of two >= max(64, 2 n)), 64 + 12 * ceil(n / 256) words and 7 *
 * n + s entries.  After ramcrc_ctx_reserve(ctx, 64 + 12 * ceil(n / 256),
 * 7 * n + s), or after any earlier call on the context that reserved as much,
 * an increment of up to n requests does not allocate.  The call is
 * stream-ordered and asynchronous; lifetime and concurrency are the table's.
 *
 * Not done: chained increments of one key within a call; several output
 * segments per call and a SEGHEADER entry; RpcResult records and
 * linearizability; index entries; STATUS_UNKNOWN_TABLET and transaction locks;
 * the single-object increment RPC's response header; any change to the table
 * itself. */
#define RAMCRC_STATUS_INVALID_OBJECT 22u        /* src/Status.h */

typedef struct ramcrc_increment_arg {
    int64_t add_int64;    /* 0: no integer addition */
    double add_double;    /* 0.0 or -0.0: no floating-point addition */
} ramcrc_increment_arg;   /* 16 bytes */

typedef struct ramcrc_increment_summary {
    uint64_t ok;
    uint64_t created;          /* of ok: written without a tombstone */
    uint64_t doesnt_exist, object_exists, wrong_version, invalid_object, bad, retry_duplicate, retry_full;
    uint64_t tombstones;       /* written */
    uint64_t allocated;        /* versions taken from next_version on */
    uint64_t next_version;     /* the caller's safeVersion after the call */
    uint64_t out_bytes;        /* the output's head */
    uint64_t object_bytes;     /* payload bytes of the written objects */
    uint64_t tombstone_bytes;  /* and of the written tombstones */
    uint64_t value_bytes;      /* 8 per OK request */
    uint64_t key_bytes;        /* keysAndValueLength - valueLength, same requests */
    uint64_t spoiled;
} ramcrc_increment_summary;

int ramcrc_replay_table_increment_device(ramcrc_replay_table* t, const void* d_keys, uint64_t keys_bytes,
                                         const ramcrc_lookup_key* d_reqs, uint64_t n_reqs,
                                         const ramcrc_increment_arg* d_args,
                                         const uint64_t* d_key_hash /* nullable */,
                                         const ramcrc_reject_rules* d_rules /* nullable: no rules */,
                                         uint64_t next_version, uint32_t timestamp,
                                         const uint64_t* d_batch_segment_id /* nullable */,
                                         void* d_out, uint32_t out_capacity, ramcrc_seg_cert* d_out_cert,
                                         void* d_parts, ramcrc_write_ref* d_refs /* nullable */,
                                         ramcrc_lookup_result* d_old /* nullable */,
                                         ramcrc_increment_summary* d_summary, void* stream);

/* The same on the host, single-threaded: host pointers, no alignment rules,
 * the same bytes.  Returns RAMCRC_OK on a spoiled table, with the outputs
 * described above. */
int ramcrc_replay_table_increment_host(ramcrc_replay_table_host* t, const void* keys, uint64_t keys_bytes,
                                       const ramcrc_lookup_key* reqs, uint64_t n_reqs,
                                       const ramcrc_increment_arg* args,
                                       const uint64_t* key_hash, const ramcrc_reject_rules* rules,
                                       uint64_t next_version, uint32_t timestamp,
                                       const uint64_t* batch_segment_id, void* out, uint32_t out_capacity,
                                       ramcrc_seg_cert* out_cert, void* parts, ramcrc_write_ref* refs,
                                       ramcrc_lookup_result* old, ramcrc_increment_summary* summary);

/* Cleaning batches out of the table: the log cleaner's relocation step
 * (LogCleaner::relocateLiveEntries, src/LogCleaner.cc:575-722, over
 * ObjectManager::relocateObject, src/ObjectManager.cc:2932-2976, and
 * relocateTombstone, :3177-3219), against the replay table.  Every write and
 * remove produces a segment that becomes a batch, and the Lifetime rule keeps
 * every batch's arrays; a clean copies the records of the victim batches that
 * the table still references into one survivor segment, re-points the table
 * to the copies, makes the survivor a batch without a walk and without an
 * insert, and retires the victims.  Every record of an added batch knows its
 * slot (its work word), so the call hashes nothing, probes nothing and
 * compares no key: its cost follows the victims, never the table.
 *
 * 1. Victims.  victims[0 .. n_victims) are batch numbers, read on the host at
 *    the call.  RAMCRC_EINVAL before any launch when n_victims is 0, a number
 *    repeats, a batch was never added or was already cleaned since the last
 *    reset, or (clean only; clean_size takes no number) max_batches numbers are
 *    in use.  Records are taken victim by victim in the order given, within a
 *    victim in record order.  Ours: the entries are not sorted by timestamp
 *    (LogCleaner.cc:557-562); the caller orders the victims.
 * 2. Live.  Record i of victim b is live exactly when it was a participant of
 *    its add and is its key's winner now: live(b) at this moment, the slot's
 *    pick names {b, i}.  This is relocateObject's test (:2953-2968) and the
 *    hashReferenceExists half of relocateTombstone (:3187-3203).  Ours: a
 *    tombstone that is not its key's winner is dropped whether or not the
 *    segment it names still exists (the reference keeps it while
 *    log.segmentExists, :3184, because its hash table holds no tombstones;
 *    here the key's winner stays in the table, and a replay of what remains
 *    gives the same answers).  A winner tombstone is always kept: the table
 *    never deletes a key.
 * 3. The survivor segment.  The live records are appended to d_out from head
 *    0 as Segment::append lays entries out, each entry -- its header byte, its
 *    length bytes, its payload -- byte for byte from the source.  No tombstone
 *    is rewritten.  *d_out_cert = {head, checksum} is what
 *    ramcrc_segments_certify_device returns for d_out.  No byte at or past the
 *    head is written.
 * 4. The survivor batch.  The call assigns the next batch number N on the
 *    host under the handle's lock, as add does (*batch, summary.batch).
 *    d_out_entries[j] = {0, offset, length, header} for survivor j in
 *    increasing offset, *d_out_n_entries the number of survivors,
 *    *d_out_status = {RAMCRC_SEG_OK, the certificate's checksum, survivors, 0}:
 *    bit for bit what ramcrc_segment_walk_device writes for d_out (one segment
 *    of out_capacity bytes) under *d_out_cert; d_out_work[j] is the survivor's
 *    slot, what an add of that walk would leave.  Batch N names d_out with
 *    n_seg = 1 and these arrays, its hashes are NULL, and its participant
 *    counts are the moved objects and tombstones with 0 malformed.  d_moved[j]
 *    (nullable) is survivor j's old {batch, record}; its new reference is
 *    {N, j} (LogEntryRelocator::getNewReference).  From the call on, the
 *    Lifetime rule covers d_out and the three arrays.
 * 5. The table.  Afterwards no slot's pick and no slot's claim names a victim.
 *    A pick that named victim record {b, i} names {N, j} and keeps its type
 *    bit.  A claim that named a victim record names the key's winner after
 *    the call, a participant of the same key in N or in a batch that stays.
 *    Versions, the key count and the safe version do not change.  Later calls
 *    treat N as any batch; it may be a victim of a later clean.  A clean, like
 *    the order of adds, changes only which of several records of identical
 *    version and type is kept.
 * 6. Retired.  Once the stream has passed the call the victims' segments,
 *    status arrays, record tables, hashes and work arrays are the caller's
 *    again.  live on a cleaned batch returns RAMCRC_EINVAL; its number is not
 *    given out again until reset; stats.batches counts numbers given out.
 * 7. Space (ours).  The survivors fit when needed_bytes <= out_capacity and
 *    needed_records <= out_entries_cap.  If not, nothing is moved, no slot
 *    word changes, and the table is spoiled as by an add past key_cap (the
 *    host has retired the victims already): the summary is {spoiled = 1,
 *    needed_bytes, needed_records, every other field 0}; d_usage is written;
 *    the certificate, status and count are not.  The sum of the victims'
 *    certificate lengths always suffices as out_capacity, the sum of their
 *    record counts as out_entries_cap; clean_size gives the exact figures.
 * 8. clean_size writes the d_usage and the summary that clean would write
 *    for these victims now, with out_bytes = needed_bytes and batch = 0, and
 *    changes nothing: no table word, no number, nothing retired.  It runs
 *    clean's own first kernels.
 * 9. On a spoiled table only the summary is written, zero with spoiled = 1,
 *    and no new refusal is raised; clean still takes its number and retires
 *    its victims on the host.
 * 10. Arguments.  RAMCRC_EINVAL before any launch for NULL t, victims or
 *    d_summary; for clean, NULL d_out_cert, d_out_status, d_out_n_entries, or
 *    d_out_entries / d_out_work with out_entries_cap > 0; d_out NULL with
 *    out_capacity > 0; d_out not 16-byte aligned; out_capacity not a multiple
 *    of 16 (it becomes a batch's stride); out_entries_cap >= 2^32; misaligned
 *    structures (8 for 64-bit fields, 16 for d_out_entries, 4 for the
 *    certificate and status).  The outputs must not overlap any batch of the
 *    table; the call cannot check this.
 * 11. Stream-ordered, asynchronous, serialised by the handle like add.
 *    Scratch comes from the context: with T the sum over the victims of
 *    ceil(entries_cap / 256), after ramcrc_ctx_reserve(ctx, 2 * (n_victims +
 *    16 + 16 * T), 0) neither call allocates.
 *
 * Not done: relocation of RpcResult and transaction records (relocate's other
 * cases, src/ObjectManager.cc:2426) -- they count as dropped_other, and a
 * master that needs them keeps them itself --; TableStats decrements; several
 * survivor segments per call; choosing victims (CleanableSegmentManager);
 * dropping a tombstone's key from the table; recycling batch numbers. */
typedef struct ramcrc_clean_usage {      /* one per victim, in the order given; 32 bytes */
    uint64_t records;                    /* min(*n_entries, entries_cap) of that batch */
    uint64_t live_objects, live_tombstones;
    uint64_t live_bytes;                 /* entry bytes of its live records: header byte, length bytes, payload */
} ramcrc_clean_usage;

typedef struct ramcrc_clean_summary {
    uint64_t victims, records;           /* batches given; their records read */
    uint64_t moved_objects, moved_tombstones;
    uint64_t object_bytes, tombstone_bytes;      /* payload bytes of the moved records */
    uint64_t dropped_objects, dropped_tombstones;/* participants that are not their key's winner */
    uint64_t dropped_other;              /* records that never took part: other types, malformed,
                                            records of a segment whose status lacks RAMCRC_SEG_OK */
    uint64_t needed_bytes, needed_records;       /* what the survivors need: sum of live_bytes, live records */
    uint64_t out_bytes;                  /* the output's head (= needed_bytes when it fit) */
    uint64_t batch;                      /* the survivor batch's number */
    uint64_t spoiled;
} ramcrc_clean_summary;

int ramcrc_replay_table_clean_size_device(ramcrc_replay_table* t, const uint32_t* victims /* host */,
                                          uint32_t n_victims, ramcrc_clean_usage* d_usage /* nullable */,
                                          ramcrc_clean_summary* d_summary, void* stream);

int ramcrc_replay_table_clean_device(ramcrc_replay_table* t, const uint32_t* victims /* host */,
                                     uint32_t n_victims, void* d_out, uint32_t out_capacity,
                                     ramcrc_seg_cert* d_out_cert, ramcrc_seg_status* d_out_status,
                                     ramcrc_seg_entry* d_out_entries, uint64_t out_entries_cap,
                                     uint64_t* d_out_n_entries, uint64_t* d_out_work,
                                     ramcrc_replay_ref* d_moved /* nullable */,
                                     ramcrc_clean_usage* d_usage /* nullable */,
                                     ramcrc_clean_summary* d_summary, uint32_t* batch /* host, nullable */,
                                     void* stream);

/* The same on the host table, single-threaded: host pointers, no alignment
 * rules, the same bytes.  Where the device form spoils the table (rule 7) the
 * host form does too and returns RAMCRC_EINVAL after writing the summary. */
int ramcrc_replay_table_clean_size_host(ramcrc_replay_table_host* t, const uint32_t* victims,
                                        uint32_t n_victims, ramcrc_clean_usage* usage,
                                        ramcrc_clean_summary* summary);
int ramcrc_replay_table_clean_host(ramcrc_replay_table_host* t, const uint32_t* victims,
                                   uint32_t n_victims, void* out, uint32_t out_capacity,
                                   ramcrc_seg_cert* out_cert, ramcrc_seg_status* out_status,
                                   ramcrc_seg_entry* out_entries, uint64_t out_entries_cap,
                                   uint64_t* out_n_entries, uint64_t* out_work,
                                   ramcrc_replay_ref* moved, ramcrc_clean_usage* usage,
                                   ramcrc_clean_summary* summary, uint32_t* batch);

/* Migrating a tablet out of the table: the source half of MIGRATE_TABLET
 * (MasterService::migrateTablet, src/MasterService.cc:1084-1225, over
 * migrateSingleLogEntry, :935-1073).  The call scans listed batches in log
 * order, keeps the objects and tombstones of one table id whose key hash lies
 * in a range, and packs them into transfer segments, each sealed with its
 * certificate.  The receiving side (receiveMigrationData, :1809-1878) is
 * ramcrc_segment_walk_device under those certificates and then
 * ramcrc_replay_table_add_device into the destination table.
 *
 * 1. Source order.  batches[0 .. n_batches) are batch numbers, read on the
 *    host at the call.  RAMCRC_EINVAL before any launch when n_batches is 0, a
 *    number repeats, or a batch was never added or was cleaned since the last
 *    reset.  Records are taken batch by batch in the order given, within a
 *    batch in record order: LogIterator's order.  The caller lists the batches
 *    of the first pass and, in a later call, those added since (phases 1 and 3
 *    of the reference).
 * 2. Selection (:945-1013).  A record is selected when it was a participant
 *    of its add (an OBJ or OBJTOMB, well formed, in a segment with
 *    RAMCRC_SEG_OK), all 64 bits of its table id equal table_id, and its
 *    record hash lies in [first_hash, last_hash], both ends included.  The
 *    record hash is the one read_hashes and enumerate use: the hash the batch
 *    was added with, or Key::getHash of the record's key where the batch has
 *    none.  first_hash > last_hash selects nothing.  By default every selected
 *    object and tombstone is sent whether or not it is its key's winner
 *    (:1016-1036 says why).  Ours: with RAMCRC_MIGRATE_LIVE_ONLY only records
 *    that are their key's winner now are sent -- clean's rule 2 unchanged, the
 *    slot's pick names {batch, record}; the others count as skipped_dead.
 *    Ours: records that never took part in their add -- RPCRESULT, PREP,
 *    PREPTOMB, TXDECISION, TXPLIST and every other type, malformed and
 *    overlong records, records of a segment without RAMCRC_SEG_OK -- are not
 *    sent and count as skipped_other; they stay with the master, as clean and
 *    add leave them aside.  The tests are made in this order (participant,
 *    table id, range, winner) and a record counts under the first it fails.
 *    Unknown flag bits are RAMCRC_EINVAL.
 * 3. Transfer segments.  Output k lies at d_out + k * out_stride, holds
 *    out_capacity bytes and starts empty.  Every sent record is laid out as
 *    Segment::append(type, payload, length) lays it out: the header byte is
 *    rebuilt with the minimal length bytes (a fresh EntryHeader), not copied
 *    from the source; the payload is the source's, byte for byte.  Greedy cut:
 *    an entry with head + 1 + lengthBytes + length > out_capacity closes the
 *    current output and opens the next.  An entry that does not fit an empty
 *    output stops the call before it (:1061-1065): too_large = 1, the cursor
 *    names it, the outputs sealed so far are valid.  d_out_certs[k] = {head,
 *    checksum} is what ramcrc_segments_certify_device returns for output k;
 *    d_out_counts[k] = {entries, objects, tombstones, 0}.  No byte at or past
 *    a head is written; outputs >= segments_used are untouched, their
 *    certificates and counts included.
 * 4. Cursor.  The call starts at record start_record of batches[start_index];
 *    {n_batches, 0} is the cursor of a finished migration.  When max_segments
 *    outputs are in use, the call stops before the first entry that would
 *    open another.  The summary's next_index / next_record name the entry the
 *    call stopped before ({n_batches, 0} and done = 1 at the end of the list);
 *    every counter covers the records from the start cursor up to that entry,
 *    so the counters of chained calls add up.  K calls of one output each,
 *    chained by the cursor, write byte for byte what one call with K outputs
 *    writes.  Where one entry stops the call for several reasons, too_large
 *    is looked at first, then d_sent, then max_segments.  RAMCRC_EINVAL for
 *    start_index > n_batches, start_index == n_batches with a record, or
 *    start_record above that batch's entries_cap.
 * 5. d_sent (nullable, sent_cap entries): for every sent entry in output order
 *    its {batch, record}; d_seg_first[k] (nullable) is the index among them of
 *    output k's first entry.  With d_sent given, the call stops before the
 *    entry that would be number sent_cap, as a full output stops it: done = 0,
 *    too_large = 0, no overflow.  sent_cap > 0 without d_sent is RAMCRC_EINVAL.
 * 6. The table is read and nothing in it changes: no table word, no batch
 *    number, nothing retired.  On a spoiled table only the summary is
 *    written, zero with spoiled = 1.
 * 7. Arguments.  RAMCRC_EINVAL before any launch for NULL t, batches or
 *    d_summary; with max_segments > 0, NULL d_out_certs or d_out_counts, or
 *    NULL d_out with out_capacity > 0; d_out not 16-byte aligned; out_capacity
 *    or out_stride not a multiple of 16 (an output can become a batch's
 *    segment at the destination); out_stride < out_capacity; out_capacity >
 *    RAMCRC_MIGRATE_MAX_CAPACITY; max_segments > RAMCRC_MIGRATE_MAX_SEGMENTS;
 *    misaligned structures (8 for 64-bit fields, 4 for certificates and
 *    counts).  The outputs must not overlap any batch of the table; the call
 *    cannot check this.
 * 8. Stream-ordered, asynchronous, serialised by the handle like add.  The
 *    launches follow n_batches, the listed batches' entries_cap and
 *    max_segments, never a count the device knows, so the call chains without
 *    a sync and can be captured.  Scratch comes from the context: with T the
 *    sum over the listed batches of ceil(entries_cap / 256), after
 *    ramcrc_ctx_reserve(ctx, 2 * (n_batches + 40 + 8 * max_segments + 8 * T),
 *    128 * T) the call does not allocate.
 *
 * Stays with the master: the TabletManager test and STATUS_UNKNOWN_TABLET,
 * prepForMigration and getHeadOfLog, LOCKED_FOR_MIGRATION and the epoch wait,
 * reassignTabletOwnership, deleteTablet and removeOrphanedObjects, the
 * transaction and RpcResult records, the transport. */
#define RAMCRC_MIGRATE_LIVE_ONLY 1u
#define RAMCRC_MIGRATE_MAX_CAPACITY (1u << 28)
#define RAMCRC_MIGRATE_MAX_SEGMENTS 65536u

typedef struct ramcrc_migrate_count {    /* one per output; 16 bytes */
    uint32_t entries, objects, tombstones, reserved;
} ramcrc_migrate_count;

typedef struct ramcrc_migrate_summary {
    uint64_t next_index, next_record;    /* the cursor of the next call */
    uint64_t done;                       /* the list is exhausted */
    uint64_t too_large;                  /* the entry at the cursor fits no empty output */
    uint64_t segments_used;
    uint64_t sent_objects, sent_tombstones;
    uint64_t sent_bytes;                 /* entry bytes: header byte, length bytes, payload */
    uint64_t payload_bytes;              /* totalBytes of :1039 */
    uint64_t records_read;               /* from the start cursor up to the next */
    uint64_t skipped_other, skipped_table, skipped_range, skipped_dead;
    uint64_t spoiled;
} ramcrc_migrate_summary;

int ramcrc_replay_table_migrate_device(ramcrc_replay_table* t, const uint32_t* batches /* host */,
                                       uint32_t n_batches, uint64_t table_id, uint64_t first_hash,
                                       uint64_t last_hash, uint32_t flags, uint32_t start_index,
                                       uint32_t start_record, void* d_out, uint32_t out_capacity,
                                       uint64_t out_stride, uint32_t max_segments,
                                       ramcrc_seg_cert* d_out_certs, ramcrc_migrate_count* d_out_counts,
                                       ramcrc_replay_ref* d_sent /* nullable */, uint64_t sent_cap,
                                       uint64_t* d_seg_first /* nullable */,
                                       ramcrc_migrate_summary* d_summary, void* stream);

/* The same on the host table, single-threaded: host pointers, no alignment
 * rules for the structures, the same bytes.  start_record is held against the
 * batch's record count. */
int ramcrc_replay_table_migrate_host(ramcrc_replay_table_host* t, const uint32_t* batches,
                                     uint32_t n_batches, uint64_t table_id, uint64_t first_hash,
                                     uint64_t last_hash, uint32_t flags, uint32_t start_index,
                                     uint32_t start_record, void* out, uint32_t out_capacity,
                                     uint64_t out_stride, uint32_t max_segments,
                                     ramcrc_seg_cert* out_certs, ramcrc_migrate_count* out_counts,
                                     ramcrc_replay_ref* sent, uint64_t sent_cap, uint64_t* seg_first,
                                     ramcrc_migrate_summary* summary);

/* The side log of a replay: what ObjectManager::replaySegment hands to
 * sideLog->append for every record it keeps (src/ObjectManager.cc:720-734,
 * :840-867), and where each record then lies.  The call is
 * ramcrc_recovery_append_device at n_part = 1 over a live list -- the {record,
 * 0} lists ramcrc_replay_resolve_device and ramcrc_replay_table_live_device
 * write -- with two additions: kept tombstones are rewritten as the reference
 * rewrites them before it logs them, and every placement gets a reference.
 *
 * Append rules.  Every rule of ramcrc_recovery_append_device at n_part = 1
 * holds unchanged: output k belongs to source segment k; entry header bytes,
 * the fit rule, d_out_certs and d_out_status, "bytes of an output at or past
 * its head are never written", the alignment rules (d_base 16-byte aligned,
 * seg_stride a multiple of 16, d_out and out_stride free, out_stride >=
 * out_capacity, live_cap < 2^32, outputs not overlapping the source),
 * stream-ordered and asynchronous.  A placement whose partition is not 0 is a
 * partition >= n_part: the call refuses.
 *
 * Refusal.  The conditions are the append's; a refused call writes none of
 * d_out, d_out_certs, d_out_status, d_refs, d_counts, and ramcrc_ctx_check
 * returns RAMCRC_EREFUSED.  With n_seg = 0 the call returns RAMCRC_OK and
 * writes nothing, as the append does.
 *
 * Tombstones.  An appended record of type OBJTOMB whose payload has at least
 * 32 bytes (ObjectTombstone::Header, src/Object.h:285-338) is written with
 *   payload [8, 16)  zero: segmentId 0, "can be cleaned as soon as the hash
 *                    table ceases to reference it" (:847-849);
 *   payload [24, 28) `timestamp`, little-endian (:845);
 *   payload [28, 32) the finalized CRC32C of the new bytes [0, 28) followed
 *                    by the key [32, length): ObjectTombstone::computeChecksum
 *                    (src/Object.cc:1042-1057), little-endian (:850-851);
 * and every other payload byte copied.  The checksum is computed from the
 * bytes, not derived from the stored one: a tombstone whose stored checksum
 * was wrong leaves with a correct one, as in the reference, where replay only
 * warns about it (:758-763).  An OBJTOMB record shorter than 32 bytes is
 * copied unchanged and counted in short_tombstones (resolution never lists
 * one, but the call takes any list).  Every other type is copied byte for
 * byte, exactly as the append copies it.
 *
 * Certificates are the append's: Segment::getAppendedLength's checksum covers
 * entry headers and the length only (src/Segment.cc:672-684), so the rewrite
 * of payload bytes does not change it.
 *
 * timestamp is passed by value: the caller reads its clock once per call, as
 * one WallTime::secondsTimestamp() would serve a segment.  A captured graph
 * replays the captured value.
 *
 * d_refs (nullable; one per entry of the live list, live_cap of them):
 * d_refs[i] = {output index, byte offset of the entry header} of the record
 * placement i appended -- the Log::Reference sideLog->append returns, for
 * replace(lock, key, reference) (:734, :867) -- or {0xFFFFFFFF, 0xFFFFFFFF}
 * when the placement was not appended (its output is RAMCRC_SEG_APPEND_FULL or
 * RAMCRC_SEG_SOURCE_BAD).  Entries at and past *d_n_live are not written.
 * d_counts (required): see the structure.
 *
 * Still not done: the synthesized tombstone for an overwritten object
 * (:697-717, :804-835), raiseSafeVersion (:797), transaction records (copied
 * like any other type when listed), and insertion into the master's table.
 * The intended use needs no synthesized tombstone: a master that asks for the
 * live lists after its last add logs only final winners, so nothing it logged
 * is ever overwritten.
 *
 * Scratch comes from the context: after ramcrc_ctx_reserve(ctx, 80 + 4 *
 * n_seg, live_cap / 2 + 1), or after one call of the same shape, it does not
 * allocate. */
typedef struct ramcrc_log_ref {
    uint32_t segment;   /* output index (= source segment) */
    uint32_t offset;    /* of the entry header in that output */
} ramcrc_log_ref;
#define RAMCRC_LOG_REF_NONE 0xFFFFFFFFu

typedef struct ramcrc_sidelog_counts {
    uint64_t objects;           /* appended OBJ records (objectAppendCount, :742) */
    uint64_t tombstones;        /* appended and rewritten (tombstoneAppendCount, :862) */
    uint64_t other;             /* appended records of every other type */
    uint64_t object_bytes;      /* payload bytes of `objects` (liveObjectBytes, TableStats: :729-743) */
    uint64_t tombstone_bytes;   /* payload bytes of `tombstones` (TableStats: :863-866) */
    uint64_t short_tombstones;  /* appended OBJTOMB records below 32 bytes: copied unchanged */
    uint64_t left_out;          /* placements not appended */
} ramcrc_sidelog_counts;

int ramcrc_replay_sidelog_device(ramcrc_ctx* ctx, const void* d_base, uint64_t seg_stride,
                                 uint64_t n_seg, const ramcrc_seg_status* d_status,
                                 const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                 const uint64_t* d_n_entries, const ramcrc_placement* d_live,
                                 uint64_t live_cap, const uint64_t* d_n_live, uint32_t timestamp,
                                 void* d_out, uint64_t out_stride, uint32_t out_capacity,
                                 ramcrc_seg_cert* d_out_certs, ramcrc_append_status* d_out_status,
                                 ramcrc_log_ref* d_refs, ramcrc_sidelog_counts* d_counts,
                                 void* stream);

/* The same on the host, single-threaded: host pointers, n_entries records,
 * n_live placements, no alignment rules.  Returns RAMCRC_EINVAL where the
 * device form refuses (nothing is written). */
int ramcrc_replay_sidelog_host(const void* base, uint64_t seg_stride, uint64_t n_seg,
                               const ramcrc_seg_status* status, const ramcrc_seg_entry* entries,
                               uint64_t n_entries, const ramcrc_placement* live, uint64_t n_live,
                               uint32_t timestamp, void* out, uint64_t out_stride,
                               uint32_t out_capacity, ramcrc_seg_cert* out_certs,
                               ramcrc_append_status* out_status, ramcrc_log_ref* refs,
                               ramcrc_sidelog_counts* counts);

/* ObjectManager::replaySegment's checksum checks for every record of a walk
 * whose segment passed the metadata check (d_status flags RAMCRC_SEG_OK;
 * records of failed segments are skipped, as RecoverySegmentBuilder::build
 * stops there):
 *   LOG_ENTRY_TYPE_OBJ          Object::computeChecksum (src/Object.cc:805-819)
 *                               over payload bytes [4, length) vs. the stored
 *                               checksum at [0, 4) (src/ObjectManager.cc:659-669);
 *   LOG_ENTRY_TYPE_OBJTOMB      ObjectTombstone::checkIntegrity
 *                               (src/ObjectManager.cc:752-758): bytes [0, 28) and
 *                               the key [32, length) vs. the checksum at [28, 32);
 *   LOG_ENTRY_TYPE_SAFEVERSION  ObjectSafeVersion::checkIntegrity
 *                               (src/ObjectManager.cc:873-880): bytes [0, 8) vs.
 *                               the checksum at [8, 12);
 *   LOG_ENTRY_TYPE_PREP         PreparedOp::checkIntegrity (src/ObjectManager.cc:956,
 *                               src/PreparedOp.cc:177-190): header bytes [0, 28)
 *                               and the object from its byte 4, [36, length), vs.
 *                               the checksum at [28, 32);
 *   LOG_ENTRY_TYPE_PREPTOMB     PreparedOpTombstone::checkIntegrity (:1013,
 *                               src/PreparedOp.cc:271-282): bytes [0, 40) vs. [40, 44);
 *   LOG_ENTRY_TYPE_TXDECISION   TxDecisionRecord::checkIntegrity (:1060,
 *                               src/TxDecisionRecord.cc:209-223): bytes [0, 44) and
 *                               24 * participantCount (uint32, at [36, 40)) bytes
 *                               from 48, clipped to the entry as Buffer::Iterator
 *                               does, vs. the checksum at [44, 48);
 *   LOG_ENTRY_TYPE_TXPLIST      ParticipantList::checkIntegrity (:1084,
 *                               src/ParticipantList.cc:96-110): bytes [0, 20) and
 *                               24 * participantCount (uint32, at [16, 20)) bytes
 *                               from 24 vs. the checksum at [20, 24); a list
 *                               longer than the entry fails (the reference's
 *                               getRange returns NULL there).
 * The computed CRC goes to d_obj_crc[i] (other records: not written), and
 * d_status[segment].bad_objects += 1 per failed check (records shorter than
 * their type's header, 24 / 32 / 12 / 56 / 44 / 48 / 24 bytes, or flagged
 * OVERLONG fail).  Objects of >= 64 KiB are scanned by all CUs, smaller ones
 * by the small-entry kernels; the other types by one thread each.  Stream-ordered
 * after the walk that produced the table. */
int ramcrc_verify_objects_device(ramcrc_ctx* ctx, const void* d_base, uint64_t seg_stride,
                                 const ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                 const uint64_t* d_n_entries, uint32_t* d_obj_crc,
                                 ramcrc_seg_status* d_status, void* stream);

/* The walk and the checks above in one call, as a recovery master replays a
 * batch of segments right after walking them (RecoverySegmentBuilder::build
 * then ObjectManager::replaySegment, src/RecoverySegmentBuilder.cc:61-203,
 * src/ObjectManager.cc:585-1115): exactly ramcrc_segment_walk_device
 * followed by ramcrc_verify_objects_device on the table it wrote (same
 * arguments, same results, same record table), with one shortcut the split
 * calls cannot take -- the walk notes whether any record it writes needs more
 * than the one-window object path (a larger object, or a tombstone, safe
 * version or transaction record), and when none does (RecoverSegmentBenchmark's
 * small-value segments) the checks skip the binning pass over the table.
 * Stream-ordered. */
int ramcrc_replay_verify_device(ramcrc_ctx* ctx, const void* d_base, uint64_t seg_stride,
                                uint32_t seg_capacity, uint64_t n_seg,
                                const ramcrc_seg_cert* d_certs, ramcrc_seg_status* d_status,
                                ramcrc_seg_entry* d_entries, uint64_t entries_cap,
                                uint64_t* d_n_entries, uint32_t* d_obj_crc, void* stream);

/* Host append path (src/Segment.cc:197-228 with src/Object.cc:213-218):
 * appends LOG_ENTRY_TYPE_OBJ entries holding objects {tableId 0, key = 8-byte
 * counter from first_key, version 0, timestamp 0, value_len value bytes} to an
 * empty segment of `capacity` bytes until the next one does not fit, as
 * RecoverSegmentBenchmark::run fills its segments
 * (nanobenchmarks/RecoverSegmentBenchmark.cc:131-146).  The value bytes are
 * whatever `seg` already holds at their positions; bytes after the last entry
 * are zeroed.  Writes the certificate (Segment::getAppendedLength,
 * src/Segment.cc:672-684) and the object count. */
int ramcrc_segment_fill_objects(uint8_t* seg, uint32_t capacity, uint32_t value_len,
                                uint64_t first_key, uint32_t* n_objects, ramcrc_seg_cert* cert);

/* Device form of ramcrc_segment_fill_objects for n_seg segments at d_base +
 * i*seg_stride (RecoverSegmentBenchmark::run's input, the BASELINE C4 shard,
 * built where it is scanned): segment i holds keys first_key + i*per ..
 * first_key + (i+1)*per - 1, per = objects per segment; value bytes are
 * whatever the segments already hold; bytes after the last entry are zeroed;
 * every Object::Header::checksum is computed by the batch kernels.  The
 * layout equals ramcrc_segment_fill_objects' byte for byte.  Every segment
 * gets the same certificate (the metadata checksum covers only entry headers
 * and lengths): written to *h_cert, to d_certs[i] when d_certs (device) is
 * not NULL, and per to *h_objects.  seg_stride >= capacity.  Synchronous. */
int ramcrc_segment_fill_objects_device(ramcrc_ctx* ctx, void* d_base, uint64_t seg_stride,
                                       uint32_t capacity, uint64_t n_seg, uint32_t value_len,
                                       uint64_t first_key, ramcrc_seg_cert* d_certs,
                                       ramcrc_seg_cert* h_cert, uint32_t* h_objects);

/* ------------------------------------------- multi-GPU recovery shard --- */

/* The recovery-scan batch sharded across GPUs: a backup's
 * replicas are verified independently (BackupMasterRecovery::
 * CyclicReplicaBuffer::buildNext, src/BackupMasterRecovery.cc:743-809), so
 * rank r of N scans the contiguous segment range ramcrc_shard_range(nseg, N,
 * r) held in its own GPU's HBM, and one RCCL all-gather of the 4-byte
 * results (the only exchange) leaves every rank with all CRCs in segment
 * order.  Segment bytes never cross xGMI.  RCCL (librccl.so.1) is loaded
 * at the first shard call; without it the shard calls return RAMCRC_ERCCL.
 *
 * Two ways to build one:
 *   ramcrc_shard_create_all  one process drives `ndev` GPUs (ncclCommInitAll);
 *                            local rank k = devices[k] = global rank k;
 *   ramcrc_shard_create_rank one process per GPU (ncclCommInitRank): every
 *                            process passes the same unique id (made by one
 *                            of them with ramcrc_shard_unique_id and sent to
 *                            the others out of band) and its own rank.
 * A shard owns one stream and one ramcrc_ctx per local rank. */
typedef struct ramcrc_shard ramcrc_shard;
#define RAMCRC_SHARD_ID_BYTES 128

int ramcrc_shard_unique_id(void* id /* RAMCRC_SHARD_ID_BYTES */);
int ramcrc_shard_create_all(const int* devices, int ndev, ramcrc_shard** out);
int ramcrc_shard_create_rank(const void* id, int nranks, int rank, int device,
                             ramcrc_shard** out);
int ramcrc_shard_destroy(ramcrc_shard* shard);

/* Contiguous [lo, hi) of segment indices owned by `rank` (sizes differ by at
 * most one; lower ranks get the extra ones).  Pure host arithmetic. */
int ramcrc_shard_range(uint64_t nseg, int nranks, int rank, uint64_t* lo, uint64_t* hi);

/* Local ranks this handle drives, and the global rank / device / stream /
 * context of local rank k (for callers that order their own work against
 * the shard, or time it with ramcrc_ctx_set_timing). */
int ramcrc_shard_local_count(const ramcrc_shard* shard);
int ramcrc_shard_info(const ramcrc_shard* shard, int k, int* rank, int* device, void** stream,
                      ramcrc_ctx** ctx);

/* One recovery-scan step.  For every local rank k (global rank r):
 * d_shard[k] (on that rank's device) holds segments [lo_r, hi_r) of the
 * batch at seg_bytes stride; after the step, d_all[k] (device, nseg uint32)
 * holds the CRCs of all nseg segments in segment order -- or, when d_all is
 * NULL, the shard's own result buffers do (ramcrc_shard_results).  flags:
 * RAMCRC_FINALIZE as for ramcrc_segments_device.  Asynchronous on the
 * shard's streams; a single-process shard issues the ranks' collectives in
 * one RCCL group.  Every rank must pass the same nseg.
 *
 * Liveness (ramcloud_amd/csrc/shard_plan.h): no rank leaves a step before a
 * collective its peers wait in.  A step whose nseg exceeds every earlier one
 * grows the shard's internal buffers on every rank and then exchanges one
 * status word per rank, synchronously; if any rank could not allocate, every
 * rank returns an error before the data collective (RAMCRC_ENOMEM on that
 * rank, RAMCRC_EPEER on the others).  Any other failure of a rank (bad
 * arguments, a failed launch) is returned by it, and it still joins the
 * all-gather with its segments' slots set to 0xFFFFFFFF; its status word
 * travels with the CRCs, so its peers' next ramcrc_shard_sync returns
 * RAMCRC_EPEER. */
int ramcrc_shard_segments(ramcrc_shard* shard, const void* const* d_shard, uint64_t seg_bytes,
                          uint64_t nseg, uint32_t* const* d_all, uint32_t flags);

/* Wait for every local rank's stream.  Returns RAMCRC_ERCCL if RCCL reported
 * an asynchronous error, a device launch's refusal (ramcrc_ctx_check), this
 * rank's own failure of the last step, RAMCRC_EPEER when the last step's
 * gathered status words show that another rank failed (the results then hold
 * 0xFFFFFFFF for its segments), RAMCRC_OK when every CRC of the last step is
 * valid.  Device-side refusals are only seen by the rank that hit them (the
 * uniform-segment scan never refuses). */
int ramcrc_shard_sync(ramcrc_shard* shard);

/* Copy local rank k's gathered CRCs of the last step (when it ran with d_all
 * == NULL) to host memory; synchronous. */
int ramcrc_shard_results(ramcrc_shard* shard, int k, uint32_t* h_out, uint64_t nseg);

/* ------------------------------------------------- batched write path --- */

/* Object::assembleForLog's checksum (src/Object.cc:213-238; the value is
 * Object::computeChecksum, src/Object.cc:770-819) for a batch of serialized
 * objects in device memory, e.g. the objects of a multi-write batch before
 * Log::append (src/ObjectManager.cc:1274-1297): object i is d_len[i] bytes at
 * d_base + d_off[i] -- Object::Header {checksum, timestamp, version, tableId}
 * (src/Object.h:137-182) followed by keysAndValue.  For every object of at
 * least the 24-byte header, the finalized CRC32C of bytes [4, len) is stored
 * little-endian into bytes [0, 4) (Header::checksum) and into d_out[i] when
 * d_out is not NULL; shorter objects are left unchanged (d_out[i] = 0).
 * Objects must not overlap.  Stream-ordered. */
int ramcrc_assemble_objects_device(ramcrc_ctx* ctx, void* d_base, const uint64_t* d_off,
                                   const uint64_t* d_len, uint32_t* d_out, uint64_t n,
                                   void* stream);

/* The same for objects in host memory (a write batch still in its RPC
 * buffers): staged through pinned memory, CRCs computed on the GPU, each
 * Header::checksum written back into the host object.  Synchronous. */
int ramcrc_assemble_objects_host(ramcrc_ctx* ctx, void* const* objs, const uint64_t* lens,
                                 uint64_t n);

/* Context options.
 *   RAMCRC_OPT_SERIAL_WALK  nonzero: ramcrc_segment_walk_device walks every
 *                           segment with one wavefront (the chain followed
 *                           hop by hop); 0 (default): the parallel walk,
 *                           which finds the chain in every 64 KiB part of a
 *                           segment at once and hands only anomalous segments
 *                           (offset wraps) to the serial walker.  Both give
 *                           identical results. */
#define RAMCRC_OPT_SERIAL_WALK 1
/*   RAMCRC_OPT_WALK_PART_SHIFT  log2 of the parallel walk's part size, 13..20
 *                           (8 KiB .. 1 MiB), forced for every batch; 0: the
 *                           default, chosen per batch from the entry density
 *                           (about 64 entries per part, 64 KiB .. 1 MiB).
 *                           Results are identical for every part size (the
 *                           parity tests run several). */
#define RAMCRC_OPT_WALK_PART_SHIFT 2
/*   RAMCRC_OPT_TEST_FAIL_AFTER_COUNT  test hook: the next `value` small-entry
 *                           launch sequences return RAMCRC_EHIP right after
 *                           their histogram pass is enqueued (the launch
 *                           failure the error paths must survive); 0: off. */
#define RAMCRC_OPT_TEST_FAIL_AFTER_COUNT 3
/*   RAMCRC_OPT_TEST_DIRTY_BINS  test hook: the next small-entry launch adds
 *                           (value & 0xffff) to the histogram count of bin
 *                           value >> 16 between its count and scatter passes;
 *                           the launch must then refuse (RAMCRC_EINTERNAL from
 *                           ramcrc_ctx_check) rather than read stale slots. */
#define RAMCRC_OPT_TEST_DIRTY_BINS 4
/*   RAMCRC_OPT_TEST_BIN_STRAGGLER  test hook: the next one-launch binning
 *                           (k_bin_one, batches of at most one 4,096-entry
 *                           tile per CU) waits for one workgroup more than it
 *                           launched, as if part of the grid were never
 *                           dispatched; it must abort after its stall period
 *                           (no arrival for 30 us) and the launch complete
 *                           through the two-launch binning with exact results. */
#define RAMCRC_OPT_TEST_BIN_STRAGGLER 5
/*   RAMCRC_OPT_BIN_ONE     small-entry batches of at most one 4,096-entry
 *                           tile per CU: 1 bins them with the one-launch
 *                           k_bin_one (a grid-wide vote), 0
 *                           (default since round 6) with the two-launch count
 *                           and scatter.  Identical results. */
#define RAMCRC_OPT_BIN_ONE 6
/*   RAMCRC_OPT_VERIFY_IN_WALK  ramcrc_replay_verify_device with small entries
 *                           (the objects of 64- and 128-byte values): 1
 *                           (default) checks each object while its record is
 *                           copied, from the object bytes staged in LDS, and
 *                           skips the binned object scan; 2 does so for every
 *                           batch; 0 always runs the binned scan.  Identical
 *                           results. */
#define RAMCRC_OPT_VERIFY_IN_WALK 7
int ramcrc_ctx_set_option(ramcrc_ctx* ctx, int option, int64_t value);

/* Kernel timing (for benchmarks): when enabled, every launch brackets its
 * byte-scan kernel (k_chunks, or k_entries on the small path; in the fused
 * replay call also the two k_walk_copyv launches, which do the object checks
 * in verify-in-walk mode) with HIP events on the launch stream.  ramcrc_ctx_scan_time waits for the recorded events,
 * returns the summed kernel milliseconds and the number of bracketed launches
 * since the last call, and resets both. */
int ramcrc_ctx_set_timing(ramcrc_ctx* ctx, int enable);
int ramcrc_ctx_scan_time(ramcrc_ctx* ctx, double* total_ms, uint64_t* launches);

/* Replay pipelining (a recovery master replaying a stream of segment batches,
 * src/ObjectManager.cc:580-1100): the segment walk is one latency-bound wave
 * per segment, the object scan a bandwidth-bound persistent grid whose
 * workgroups take most of a CU's LDS, so the two cannot share CUs.
 * ramcrc_stream_create_cu_mask creates a stream whose kernels run only on
 * the CUs set in cu_mask (hipExtStreamCreateWithCUMask; bit i of word i/32 =
 * CU i, mask_words <= 8); ramcrc_ctx_set_cus(ctx, n) sizes the context's
 * persistent grids (k_chunks, k_entries*) for n CUs (0 = all of them), to
 * match the mask of the stream the context launches on.  Walking batch k on
 * one masked stream while batch k-1 is scanned on the complementary one
 * overlaps the two. */
int ramcrc_stream_create_cu_mask(int device, const uint32_t* cu_mask, uint32_t mask_words,
                                 void** out_stream);
int ramcrc_stream_destroy(void* stream);
int ramcrc_ctx_set_cus(ramcrc_ctx* ctx, int ncu);

/* Raw launch status word of the context (bit 0: the latest planned launch
 * found more chunks than the scratch holds and wrote none of its outputs;
 * bit 1: some launch refused since the last ramcrc_ctx_check; bit 2: one of
 * them was a small-entry launch whose bin layout was inconsistent).
 * Synchronous. */
int ramcrc_ctx_status(ramcrc_ctx* ctx, uint32_t* status);

/* Waits for `stream`, then returns RAMCRC_EINTERNAL or RAMCRC_EREFUSED (and
 * clears the sticky bits, atomically on the device) if any launch of this
 * context was refused since the last check, RAMCRC_OK otherwise.  A refusal
 * needs a general batch whose buffers
 * overlap or total more bytes than the device holds (ramcrc_batch_device,
 * ramcrc_verify_objects_device, ramcrc_assemble_objects_device); raise
 * ramcrc_ctx_reserve and retry.  ramcrc_recovery_append_device refuses a
 * placement list that breaks its rules: correct the list;
 * ramcrc_recovery_partition_device a tablet whose partition is out of range
 * or a record table that is not a walk's.  The host entry points (ramcrc_batch_host,
 * ramcrc_assemble_objects_host) check by themselves. */
int ramcrc_ctx_check(ramcrc_ctx* ctx, void* stream);

/* Diagnostics.  ramcrc_ctx_debug_bins waits for the device and copies the
 * small-entry bin table's counts, both counter copies' cursors and
 * histograms (5 x 161 words), then the number of one-launch binnings that
 * aborted and completed through the two-launch path (1 word), to host, and
 * the parity of the next sequence. */
int ramcrc_ctx_debug_bins(ramcrc_ctx* ctx, uint64_t* host, uint64_t nwords, uint32_t* par_next);
const char* ramcrc_strerror(int code);
int ramcrc_last_hip_error(void);            /* last hipError_t seen (thread-local) */
int ramcrc_device_count(void);
const char* ramcrc_build_info(void);

#ifdef __cplusplus
}
#endif

#endif /* RAMCRC_H */
