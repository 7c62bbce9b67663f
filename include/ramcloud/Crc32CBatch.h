/* Opt-in batch CRC32C on an MI355X for RAMCloud callers that hold many
 * independent buffers at once:
 *
 *   - the backup recovery scan: every loaded replica frame is a contiguous
 *     8 MiB buffer (BackupStorage::Frame::load, src/BackupStorage.h:227)
 *     verified independently in BackupMasterRecovery::CyclicReplicaBuffer::
 *     buildNext (src/BackupMasterRecovery.cc:743-809);
 *   - the recovery-master replay: one Object::computeChecksum per object of a
 *     recovery segment (src/ObjectManager.cc:659-663, src/Object.cc:805-819).
 *
 * Each call returns exactly what `Crc32C c; c.update(buf_i, len_i);
 * c.getResult()` returns for every buffer (or the raw running value, for
 * chaining), computed by libramcrc's gfx950 kernels.  Comparison against the
 * stored checksums stays with the caller, as in the reference
 * (src/Segment.cc:793-797, src/ObjectManager.cc:664-669).
 *
 * Errors from the C ABI (include/ramcrc.h) become RAMCRC_BATCH_THROW(msg),
 * which is `throw FatalError(HERE, msg)` inside RAMCloud (src/Exception.h:70)
 * and std::runtime_error elsewhere.  No HIP header is needed by callers.
 */
#ifndef RAMCLOUD_CRC32CBATCH_H
#define RAMCLOUD_CRC32CBATCH_H

#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "ramcrc.h"

#ifndef RAMCRC_BATCH_THROW
#if defined(RAMCLOUD_EXCEPTION_H)
#define RAMCRC_BATCH_THROW(msg) throw RAMCloud::FatalError(HERE, msg)
#else
#include <stdexcept>
#define RAMCRC_BATCH_THROW(msg) throw std::runtime_error(msg)
#endif
#endif

namespace RAMCloud {

class Crc32CBatch {
  public:
    /// Binds to a GPU lazily on first use (never at static-init time).
    explicit Crc32CBatch(int device = 0)
        : device(device)
        , ctx(NULL)
    {
    }

    ~Crc32CBatch()
    {
        if (ctx)
            ramcrc_ctx_destroy(ctx);
    }

    /**
     * CRC32C of host buffers (e.g. loaded replica frames): staged through
     * pinned memory to the GPU and back.  Synchronous.
     * \param buffers
     *      (pointer, length) of every buffer.
     * \param finalize
     *      true: getResult() values; false: raw running values.
     */
    std::vector<uint32_t>
    hostBuffers(const std::vector<std::pair<const void*, uint64_t> >& buffers,
                bool finalize = true)
    {
        std::vector<const void*> ptrs;
        std::vector<uint64_t> lens;
        for (size_t i = 0; i < buffers.size(); i++) {
            ptrs.push_back(buffers[i].first);
            lens.push_back(buffers[i].second);
        }
        std::vector<uint32_t> out(buffers.size());
        if (!buffers.empty())
            check(ramcrc_batch_host(context(), &ptrs[0], &lens[0], NULL, &out[0],
                                    out.size(), finalize ? RAMCRC_FINALIZE : 0u),
                  "ramcrc_batch_host");
        return out;
    }

    /// Device-resident uniform segments (the recovery-scan batch): d_out[i]
    /// for segment i = d_base + i * segmentBytes.  With wait (the default)
    /// the call returns after the results are in d_out; wait = false leaves
    /// it asynchronous on `stream`, to be followed by sync(stream).
    void
    deviceSegments(const void* d_base, uint64_t segmentBytes, uint64_t count,
                   uint32_t* d_out, void* stream = NULL, bool finalize = true, bool wait = true)
    {
        check(ramcrc_segments_device(context(), d_base, segmentBytes, count, NULL, d_out,
                                     finalize ? RAMCRC_FINALIZE : 0u, stream),
              "ramcrc_segments_device");
        if (wait)
            sync(stream);
    }

    /// Device-resident (offset, length) table, e.g. the (off + 4, len - 4)
    /// object ranges of a recovery segment.  wait: as for deviceSegments.
    /// A batch the context's scratch cannot plan (overlapping buffers
    /// totalling more than the device holds) throws instead of leaving
    /// d_out unwritten.
    void
    deviceBatch(const void* d_base, const uint64_t* d_off, const uint64_t* d_len,
                const uint32_t* d_init, uint32_t* d_out, uint64_t count, void* stream = NULL,
                bool finalize = true, bool wait = true)
    {
        check(ramcrc_batch_device(context(), d_base, d_off, d_len, d_init, d_out, count,
                                  finalize ? RAMCRC_FINALIZE : 0u, stream),
              "ramcrc_batch_device");
        if (wait)
            sync(stream);
    }

    /// Waits for `stream` and throws if a launch of this object was refused
    /// since the last sync (ramcrc_ctx_check): the outputs of a refused
    /// launch are not written, and an integrity path must not read them.
    void
    sync(void* stream = NULL)
    {
        check(ramcrc_ctx_check(context(), stream), "ramcrc_ctx_check");
    }

    /**
     * The checks a recovery master makes on a batch of replicas resident in
     * HBM: Segment::checkMetadataIntegrity of every segment
     * (src/Segment.cc:758-800), then every checkIntegrity replaySegment makes
     * on the entries of the segments that passed (src/ObjectManager.cc:580-1100).
     * Segment i = d_base + i * stride, `capacity` bytes.  d_status[i] gets the
     * flags, metadata checksum, entry count and failed checks; d_entries /
     * d_objCrc the walked records and their computed CRCs.  Returns after
     * both kernels finished on `stream` (see ramcrc_segment_walk_device /
     * ramcrc_verify_objects_device).  A segment whose records did not fit
     * in entriesCap carries RAMCRC_SEG_TABLE_FULL and never RAMCRC_SEG_OK:
     * it was not verified; walk it again with a larger table.
     */
    void
    deviceReplayVerify(const void* d_base, uint64_t stride, uint32_t capacity, uint64_t count,
                       const ramcrc_seg_cert* d_certs, ramcrc_seg_status* d_status,
                       ramcrc_seg_entry* d_entries, uint64_t entriesCap, uint64_t* d_nEntries,
                       uint32_t* d_objCrc, void* stream = NULL)
    {
        // walk + checks in one call (ramcrc_replay_verify_device): the same as
        // ramcrc_segment_walk_device then ramcrc_verify_objects_device
        check(ramcrc_replay_verify_device(context(), d_base, stride, capacity, count, d_certs,
                                          d_status, d_entries, entriesCap, d_nEntries, d_objCrc,
                                          stream),
              "ramcrc_replay_verify_device");
        sync(stream);
    }

    /**
     * The append loop of RecoverySegmentBuilder::build
     * (src/RecoverySegmentBuilder.cc:61-203) for the replicas a
     * deviceReplayVerify (or a walk) left in HBM: placement {record,
     * partition} appends that record of d_entries to recovery segment
     * (record's segment) * partitions + partition, which lies at d_out + that
     * index * outStride and holds outCapacity bytes.  d_outCerts gets every
     * recovery segment's certificate (Segment::getAppendedLength,
     * src/Segment.cc:672-684) and d_outStatus its flags and entry count: see
     * ramcrc_recovery_append_device.  The placement list must not decrease in
     * `record`.  Returns after the kernels finished on `stream`; throws when
     * the list was refused (nothing is written then).
     */
    void
    deviceRecoveryAppend(const void* d_base, uint64_t stride, uint64_t count,
                         const ramcrc_seg_status* d_status, const ramcrc_seg_entry* d_entries,
                         uint64_t entriesCap, const uint64_t* d_nEntries,
                         const ramcrc_placement* d_place, uint64_t placeCap,
                         const uint64_t* d_nPlace, uint32_t partitions, void* d_out,
                         uint64_t outStride, uint32_t outCapacity, ramcrc_seg_cert* d_outCerts,
                         ramcrc_append_status* d_outStatus, void* stream = NULL)
    {
        check(ramcrc_recovery_append_device(context(), d_base, stride, count, d_status, d_entries,
                                            entriesCap, d_nEntries, d_place, placeCap, d_nPlace,
                                            partitions, d_out, outStride, outCapacity, d_outCerts,
                                            d_outStatus, stream),
              "ramcrc_recovery_append_device");
        sync(stream);
    }

    /**
     * The placement decision of RecoverySegmentBuilder::build
     * (src/RecoverySegmentBuilder.cc:74-201) for the records a
     * deviceReplayVerify (or a walk) left in HBM: Key::getHash, whichPartition
     * over d_tablets (the RecoveryPartition's tablets in list order, partition =
     * user_data) and isEntryAlive.  Writes the {record, partition} list and its
     * length to d_place / d_nPlace, which deviceRecoveryAppend takes as they
     * are, the per-replica flags and counters to d_partStatus and, when
     * d_keyHash is not NULL, every record's key hash: see
     * ramcrc_recovery_partition_device.  Returns after the kernels finished on
     * `stream`; throws when the call was refused (a tablet's partition >=
     * partitions, a record table that is not a walk's).
     */
    void
    deviceRecoveryPartition(const void* d_base, uint64_t stride, uint64_t count,
                            const ramcrc_seg_status* d_status, const ramcrc_seg_entry* d_entries,
                            uint64_t entriesCap, const uint64_t* d_nEntries,
                            const ramcrc_tablet* d_tablets, uint32_t tablets, uint32_t partitions,
                            ramcrc_placement* d_place, uint64_t placeCap, uint64_t* d_nPlace,
                            uint64_t* d_keyHash, ramcrc_partition_status* d_partStatus,
                            void* stream = NULL)
    {
        check(ramcrc_recovery_partition_device(context(), d_base, stride, count, d_status,
                                               d_entries, entriesCap, d_nEntries, d_tablets,
                                               tablets, partitions, d_place, placeCap, d_nPlace,
                                               d_keyHash, d_partStatus, stream),
              "ramcrc_recovery_partition_device");
        sync(stream);
    }

    /**
     * On a recovery master: the decision ObjectManager::replaySegment makes
     * after each checksum (src/ObjectManager.cc:671-734, :766-867) for the
     * objects and tombstones a deviceReplayVerify (or a walk) left in HBM.
     * Per key the highest version is kept, a tombstone before an object of the
     * same version.  d_winner (nullable) receives every participant's winner
     * (a record is live when d_winner[i] == i, RAMCRC_RESOLVE_NONE for records
     * that take no part), d_live / d_nLive the live records as the {record, 0}
     * list deviceRecoveryAppend takes with partitions = 1, d_counts the
     * counters and the recovered safe version.  d_keyHash is
     * deviceRecoveryPartition's output for the same table, or NULL to have
     * the hashes computed: see ramcrc_replay_resolve_device.  The call decides
     * and inserts nothing.  Returns after the kernels finished on `stream`;
     * throws when the call was refused (a record table that names a replica
     * >= count).
     */
    void
    deviceReplayResolve(const void* d_base, uint64_t stride, uint64_t count,
                        const ramcrc_seg_status* d_status, const ramcrc_seg_entry* d_entries,
                        uint64_t entriesCap, const uint64_t* d_nEntries,
                        const uint64_t* d_keyHash, uint32_t* d_winner, ramcrc_placement* d_live,
                        uint64_t liveCap, uint64_t* d_nLive, ramcrc_resolve_counts* d_counts,
                        void* stream = NULL)
    {
        check(ramcrc_replay_resolve_device(context(), d_base, stride, count, d_status, d_entries,
                                           entriesCap, d_nEntries, d_keyHash, d_winner, d_live,
                                           liveCap, d_nLive, d_counts, stream),
              "ramcrc_replay_resolve_device");
        sync(stream);
    }

    /**
     * On a recovery master: what ObjectManager::replaySegment hands to
     * sideLog->append for every record it keeps (src/ObjectManager.cc:720-734,
     * :840-867).  d_live / d_nLive is deviceReplayResolve's or
     * ReplayTable::live's list; side-log segment k lies at d_out + k *
     * outStride, holds outCapacity bytes and receives the kept records of
     * replica k as deviceRecoveryAppend with one partition writes them, except
     * that every kept tombstone leaves as the reference rewrites it (:845-851):
     * segmentId 0, `timestamp` (one WallTime::secondsTimestamp() per call),
     * and ObjectTombstone::computeChecksum over the new bytes.  d_refs
     * (nullable) receives for placement i the Log::Reference of its record --
     * {side-log segment, offset of the entry header} -- for the hash table's
     * replace(), or RAMCRC_LOG_REF_NONE twice when it was not appended;
     * d_counts the append counts and byte sums: see
     * ramcrc_replay_sidelog_device.  Returns after the kernels finished on
     * `stream`; throws when the list was refused (nothing is written then).
     */
    void
    deviceReplaySideLog(const void* d_base, uint64_t stride, uint64_t count,
                        const ramcrc_seg_status* d_status, const ramcrc_seg_entry* d_entries,
                        uint64_t entriesCap, const uint64_t* d_nEntries,
                        const ramcrc_placement* d_live, uint64_t liveCap, const uint64_t* d_nLive,
                        uint32_t timestamp, void* d_out, uint64_t outStride, uint32_t outCapacity,
                        ramcrc_seg_cert* d_outCerts, ramcrc_append_status* d_outStatus,
                        ramcrc_log_ref* d_refs, ramcrc_sidelog_counts* d_counts,
                        void* stream = NULL)
    {
        check(ramcrc_replay_sidelog_device(context(), d_base, stride, count, d_status, d_entries,
                                           entriesCap, d_nEntries, d_live, liveCap, d_nLive,
                                           timestamp, d_out, outStride, outCapacity, d_outCerts,
                                           d_outStatus, d_refs, d_counts, stream),
              "ramcrc_replay_sidelog_device");
        sync(stream);
    }

    /**
     * Object::assembleForLog's checksum for a batch of serialized objects
     * (the write path, src/ObjectManager.cc:1274): header.checksum of every
     * object (Object::Header + keysAndValue, src/Object.h:137-182) is set to
     * Object::computeChecksum() (src/Object.cc:770-819), computed on the GPU.
     * Objects shorter than the header are left unchanged.  Synchronous.
     */
    void
    assembleObjects(const std::vector<std::pair<void*, uint64_t> >& objects)
    {
        std::vector<void*> ptrs;
        std::vector<uint64_t> lens;
        for (size_t i = 0; i < objects.size(); i++) {
            ptrs.push_back(objects[i].first);
            lens.push_back(objects[i].second);
        }
        if (!objects.empty())
            check(ramcrc_assemble_objects_host(context(), &ptrs[0], &lens[0], ptrs.size()),
                  "ramcrc_assemble_objects_host");
    }

  private:
    ramcrc_ctx*
    context()
    {
        if (!ctx)
            check(ramcrc_ctx_create(device, &ctx), "ramcrc_ctx_create");
        return ctx;
    }

    static void
    check(int rc, const char* what)
    {
        if (rc != RAMCRC_OK)
            RAMCRC_BATCH_THROW(std::string(what) + ": " + ramcrc_strerror(rc));
    }

    int device;
    ramcrc_ctx* ctx;

    friend class ReplayTable;

    Crc32CBatch(const Crc32CBatch&);             // not copyable
    Crc32CBatch& operator=(const Crc32CBatch&);
};

/**
 * deviceReplayResolve's decision fed batch by batch: a table on the GPU that
 * outlives a call (ramcrc_replay_table_*, the rules are in include/ramcrc.h).
 * MasterService::recover (src/MasterService.cc:3501-3720) calls add() for
 * every recovery segment, or group of them, as it arrives and has been
 * verified, and at the end live() and Crc32CBatch::deviceRecoveryAppend with
 * one partition for every batch.  Every array given to add() stays allocated
 * and unchanged until reset() or the table's destruction.  The table belongs
 * to `batch`'s context and must be destroyed before it.  add(), live() and
 * stats() are asynchronous on `stream`; Crc32CBatch::sync(stream) waits and
 * throws if the table was spoiled.  Errors throw like Crc32CBatch's.
 */
class ReplayTable {
  public:
    ReplayTable(Crc32CBatch& batch, uint64_t keyCap, uint32_t maxBatches)
        : table(NULL), ctx(batch.context())
    {
        check(ramcrc_replay_table_create(ctx, keyCap, maxBatches, &table),
              "ramcrc_replay_table_create");
    }

    ~ReplayTable()
    {
        if (table)
            ramcrc_replay_table_destroy(table);
    }

    /// Empties the table and forgets its batches; stream-ordered.
    void
    reset(void* stream = NULL)
    {
        check(ramcrc_replay_table_reset(table, stream), "ramcrc_replay_table_reset");
    }

    /// Resolves one walk's records into the table; d_work: entriesCap 64-bit
    /// words of the caller's, which live() reads.  Returns the batch number.
    uint32_t
    add(const void* d_base, uint64_t stride, uint64_t count, const ramcrc_seg_status* d_status,
        const ramcrc_seg_entry* d_entries, uint64_t entriesCap, const uint64_t* d_nEntries,
        const uint64_t* d_keyHash, uint64_t* d_work, void* stream = NULL)
    {
        uint32_t batch = 0;
        check(ramcrc_replay_table_add_device(table, d_base, stride, count, d_status, d_entries,
                                             entriesCap, d_nEntries, d_keyHash, d_work, &batch,
                                             stream),
              "ramcrc_replay_table_add_device");
        return batch;
    }

    /// The verdict on one batch as the table stands now: d_winner (nullable),
    /// the {record, 0} list deviceRecoveryAppend takes with one partition over
    /// that batch's segments, and the counters.
    void
    live(uint32_t batch, ramcrc_replay_ref* d_winner, ramcrc_placement* d_live, uint64_t liveCap,
         uint64_t* d_nLive, ramcrc_resolve_counts* d_counts, void* stream = NULL)
    {
        check(ramcrc_replay_table_live_device(table, batch, d_winner, d_live, liveCap, d_nLive,
                                              d_counts, stream),
              "ramcrc_replay_table_live_device");
    }

    /// Keys, winners, safe version and batches of the whole table.
    void
    stats(ramcrc_replay_table_stats* d_stats, void* stream = NULL)
    {
        check(ramcrc_replay_table_stats_device(table, d_stats, stream),
              "ramcrc_replay_table_stats_device");
    }

    /// What the table holds for each of nQueries keys as it stands now, the
    /// batched ObjectManager::lookup / readObject of MasterService::multiRead
    /// (src/MasterService.cc:1352-1415): per key the winner's {batch, record},
    /// version and kind, and for an object where its value lies in that
    /// batch's segments.  d_keyHash and d_counts are nullable.  Read-only on
    /// the table.
    void
    lookup(const void* d_keys, uint64_t keysBytes, const ramcrc_lookup_key* d_queries,
           uint64_t nQueries, const uint64_t* d_keyHash, ramcrc_lookup_result* d_results,
           ramcrc_lookup_counts* d_counts, void* stream = NULL)
    {
        check(ramcrc_replay_table_lookup_device(table, d_keys, keysBytes, d_queries, nQueries,
                                                d_keyHash, d_results, d_counts, stream),
              "ramcrc_replay_table_lookup_device");
    }

    /// The reply of MasterService::multiRead (src/MasterService.cc:1352-1415)
    /// for nQueries keys, packed on the device: per key the lookup above, the
    /// query's RejectRules as ObjectManager::rejectOperation applies them, a
    /// MultiOp::Response::ReadPart header and, for STATUS_OK, the object's
    /// keys and value (valueOnly: its value), back to back from d_reply until
    /// the next part would pass replyCap (maxResponseRpcLen less the 8 bytes
    /// of MultiOp::Response).  d_summary->returned is respHdr->count.
    /// d_keyHash, d_rules, d_partOff and d_results are nullable.  Read-only
    /// on the table; d_reply must not overlap an added batch.
    void
    multiRead(const void* d_keys, uint64_t keysBytes, const ramcrc_lookup_key* d_queries,
              uint64_t nQueries, const uint64_t* d_keyHash, const ramcrc_reject_rules* d_rules,
              bool valueOnly, void* d_reply, uint64_t replyCap, uint64_t* d_partOff,
              ramcrc_lookup_result* d_results, ramcrc_read_summary* d_summary, void* stream = NULL)
    {
        check(ramcrc_replay_table_read_device(table, d_keys, keysBytes, d_queries, nQueries,
                                              d_keyHash, d_rules,
                                              valueOnly ? RAMCRC_READ_VALUE_ONLY : 0u, d_reply,
                                              replyCap, d_partOff, d_results, d_summary, stream),
              "ramcrc_replay_table_read_device");
    }

    /// The reply of MasterService::readHashes (src/MasterService.cc:797-809)
    /// over ObjectManager::readHashes (src/ObjectManager.cc:179-265), packed
    /// on the device: for each of the nHashes primary-key hashes an
    /// IndexLookup got from its indexlet, every object of tableId whose
    /// primary-key hash equals it, as {u64 version, u32 length} and the
    /// object's keys and value, back to back from d_reply.  A hash is answered
    /// while the reply so far is at most maxLength (maxResponseRpcLen less
    /// sizeof(WireFormat::ReadHashes::Response)) and its parts end within
    /// replyCapacity.  d_summary->hashes is respHdr->numHashes and
    /// d_summary->objects the objects in the reply.  d_parts is nullable.
    /// Read-only on the table; d_reply must not overlap an added batch.
    void
    readHashes(uint64_t tableId, const uint64_t* d_hashes, uint64_t nHashes, void* d_reply,
               uint64_t replyCapacity, uint64_t maxLength, ramcrc_hash_part* d_parts,
               ramcrc_read_hashes_summary* d_summary, void* stream = NULL)
    {
        check(ramcrc_replay_table_read_hashes_device(table, tableId, d_hashes, nHashes, 0u, d_reply,
                                                     replyCapacity, maxLength, d_parts, d_summary,
                                                     stream),
              "ramcrc_replay_table_read_hashes_device");
    }

    /// One reply of MasterService::enumerate (src/MasterService.cc:409-456)
    /// over Enumeration::complete (src/Enumeration.cc:269-351), packed on the
    /// device: the objects of tableId whose key hash lies in [firstHash,
    /// lastHash] (requestedTabletStartHash, the top frame's tabletEndHash) and
    /// that none of the nStale stale frames (host memory, read before the call
    /// returns) hides, bucket by bucket from the top frame's cursor
    /// (bucketIndex, bucketNextHash) up to bucketLimit (0: the whole table), as
    /// {u32 length, log entry} entries that end within maxBytes
    /// (maxPayloadBytes less what the reply already holds) and
    /// payloadCapacity; with keysOnly an entry ends before its value.
    /// d_summary->num_buckets, next_bucket and next_hash are the top frame to
    /// serialise; when next_bucket == num_buckets with nothing sent the caller
    /// pops frames and returns tabletEndHash + 1.  Read-only on the table;
    /// d_payload must not overlap an added batch.
    void
    enumerate(uint64_t tableId, uint64_t firstHash, uint64_t lastHash, uint64_t bucketIndex,
              uint64_t bucketNextHash, uint64_t bucketLimit, const ramcrc_enum_frame* stale,
              uint32_t nStale, bool keysOnly, void* d_payload, uint64_t payloadCapacity,
              uint64_t maxBytes, ramcrc_enumerate_summary* d_summary, void* stream = NULL)
    {
        check(ramcrc_replay_table_enumerate_device(table, tableId, firstHash, lastHash, bucketIndex,
                                                   bucketNextHash, bucketLimit, stale, nStale,
                                                   keysOnly ? RAMCRC_ENUM_KEYS_ONLY : 0u, d_payload,
                                                   payloadCapacity, maxBytes, d_summary, stream),
              "ramcrc_replay_table_enumerate_device");
    }

    /// An indexlet's entries from the table, sorted on the device: for every
    /// object of tableId that the table holds now, its key indexId (>= 1, non
    /// empty: the keys MasterService::requestInsertIndexEntries sends,
    /// src/MasterService.cc:1993-2032) with the hash of its primary key, in
    /// the B-tree's order (key, then hash).  d_entries and d_hashes hold
    /// entryCapacity entries, d_indexKeys the index's own copy of its keys;
    /// with all three NULL and both capacities 0 the call only sizes
    /// (d_summary->entries_needed, key_bytes_needed).  The index is rebuilt,
    /// not edited, and stays usable, merely stale, across later adds and
    /// cleans.  Read-only on the table.
    void
    buildIndex(uint64_t tableId, uint8_t indexId, ramcrc_index_entry* d_entries,
               uint64_t entryCapacity, uint64_t* d_hashes, void* d_indexKeys, uint64_t keysCapacity,
               ramcrc_index_build_summary* d_summary, void* stream = NULL)
    {
        check(ramcrc_replay_table_index_build_device(table, tableId, indexId, d_entries, entryCapacity,
                                                     d_hashes, d_indexKeys, keysCapacity, d_summary,
                                                     stream),
              "ramcrc_replay_table_index_build_device");
    }

    /// A batch of IndexletManager::lookupIndexKeys
    /// (src/IndexletManager.cc:611-709) over the arrays buildIndex wrote, on
    /// the table's context: per query the hashes of the entries from {first
    /// key, firstAllowedKeyHash} through the last key, at most max_hashes of
    /// them, packed back to back in d_outHashes -- what readHashes takes --,
    /// and the next key and hash to go on with (nextKeyLength, nextKeyHash)
    /// when there are more.  Which indexlet owns a key, and
    /// STATUS_UNKNOWN_INDEXLET, stay with the caller.  Stream-ordered after the
    /// build: the number of entries is read from d_buildSummary on the device.
    void
    lookupIndexKeys(const ramcrc_index_entry* d_entries, const uint64_t* d_hashes,
                    const void* d_indexKeys, const ramcrc_index_build_summary* d_buildSummary,
                    const void* d_qkeys, uint64_t qkeysBytes, const ramcrc_index_query* d_queries,
                    uint64_t nQueries, uint64_t* d_outHashes, uint64_t outCapacity,
                    ramcrc_index_result* d_results, ramcrc_index_lookup_summary* d_summary,
                    void* stream = NULL)
    {
        check(ramcrc_index_lookup_device(ctx, d_entries, d_hashes, d_indexKeys, d_buildSummary, d_qkeys,
                                         qkeysBytes, d_queries, nQueries, d_outHashes, outCapacity,
                                         d_results, d_summary, stream),
              "ramcrc_index_lookup_device");
    }

    /// MasterService::multiWrite (src/MasterService.cc:1523-1601) for nReqs
    /// keysAndValue images, on the device: per request the lookup above, the
    /// RejectRules, the new version as ObjectManager::writeObject chooses it
    /// (nextVersion: segmentManager.safeVersion), then the object with its
    /// checksum and the tombstone of the object it replaces, appended to d_out
    /// as Segment::append writes them.  d_parts is the reply's body, nReqs
    /// packed MultiOp::Response::WritePart; *d_outCert seals d_out.  The table
    /// is not changed: walk d_out with *d_outCert and add() it as the next
    /// batch.  d_summary->next_version is the safeVersion to go on with.
    /// d_keyHash, d_rules, d_batchSegmentId, d_refs and d_old are nullable.
    /// d_out must not overlap an input.
    void
    multiWrite(const void* d_data, uint64_t dataBytes, const ramcrc_write_req* d_reqs,
               uint64_t nReqs, const uint64_t* d_keyHash, const ramcrc_reject_rules* d_rules,
               uint64_t nextVersion, uint32_t timestamp, const uint64_t* d_batchSegmentId,
               void* d_out, uint32_t outCapacity, ramcrc_seg_cert* d_outCert, void* d_parts,
               ramcrc_write_ref* d_refs, ramcrc_lookup_result* d_old,
               ramcrc_write_summary* d_summary, void* stream = NULL)
    {
        check(ramcrc_replay_table_write_device(table, d_data, dataBytes, d_reqs, nReqs, d_keyHash,
                                               d_rules, nextVersion, timestamp, d_batchSegmentId,
                                               d_out, outCapacity, d_outCert, d_parts, d_refs,
                                               d_old, d_summary, stream),
              "ramcrc_replay_table_write_device");
    }

    /// MasterService::multiRemove (src/MasterService.cc:1435-1505) for nReqs
    /// keys, on the device: per request the lookup above and the RejectRules
    /// as ObjectManager::removeObject applies them, then the tombstone of the
    /// object it removes, appended to d_out as Segment::append writes it.
    /// d_parts is the reply's body, nReqs packed
    /// MultiOp::Response::RemovePart; *d_outCert seals d_out.  The table is
    /// not changed: walk d_out with *d_outCert and add() it as the next batch.
    /// d_summary->next_version is the safeVersion to go on with; d_old says
    /// where each removed object lies.  d_keyHash, d_rules, d_batchSegmentId,
    /// d_refs and d_old are nullable.  d_out must not overlap an input.
    void
    multiRemove(const void* d_keys, uint64_t keysBytes, const ramcrc_lookup_key* d_reqs,
                uint64_t nReqs, const uint64_t* d_keyHash, const ramcrc_reject_rules* d_rules,
                uint64_t nextVersion, uint32_t timestamp, const uint64_t* d_batchSegmentId,
                void* d_out, uint32_t outCapacity, ramcrc_seg_cert* d_outCert, void* d_parts,
                uint32_t* d_refs, ramcrc_lookup_result* d_old, ramcrc_remove_summary* d_summary,
                void* stream = NULL)
    {
        check(ramcrc_replay_table_remove_device(table, d_keys, keysBytes, d_reqs, nReqs, d_keyHash,
                                                d_rules, nextVersion, timestamp, d_batchSegmentId,
                                                d_out, outCapacity, d_outCert, d_parts, d_refs,
                                                d_old, d_summary, stream),
              "ramcrc_replay_table_remove_device");
    }

    /// MasterService::multiIncrement (src/MasterService.cc:1277-1330) for
    /// nReqs keys, on the device: per request the lookup above and the
    /// RejectRules as MasterService::incrementObject applies them, the key's
    /// 8-byte value read out of the added segments (zero for a key without an
    /// object), d_args[q]'s integer and then its double added to it, and from
    /// there multiWrite's steps for the object that holds the new value: the
    /// version, the object with its checksum and the tombstone of the object
    /// it replaces, appended to d_out.  d_parts is the reply's body, nReqs
    /// packed MultiOp::Response::IncrementPart; *d_outCert seals d_out.  The
    /// table is not changed: walk d_out with *d_outCert and add() it as the
    /// next batch; several increments of one key go into several calls.
    /// d_summary->next_version is the safeVersion to go on with.  d_keyHash,
    /// d_rules, d_batchSegmentId, d_refs and d_old are nullable.  d_out must
    /// not overlap an input.
    void
    multiIncrement(const void* d_keys, uint64_t keysBytes, const ramcrc_lookup_key* d_reqs,
                   uint64_t nReqs, const ramcrc_increment_arg* d_args, const uint64_t* d_keyHash,
                   const ramcrc_reject_rules* d_rules, uint64_t nextVersion, uint32_t timestamp,
                   const uint64_t* d_batchSegmentId, void* d_out, uint32_t outCapacity,
                   ramcrc_seg_cert* d_outCert, void* d_parts, ramcrc_write_ref* d_refs,
                   ramcrc_lookup_result* d_old, ramcrc_increment_summary* d_summary,
                   void* stream = NULL)
    {
        check(ramcrc_replay_table_increment_device(table, d_keys, keysBytes, d_reqs, nReqs, d_args,
                                                   d_keyHash, d_rules, nextVersion, timestamp,
                                                   d_batchSegmentId, d_out, outCapacity, d_outCert,
                                                   d_parts, d_refs, d_old, d_summary, stream),
              "ramcrc_replay_table_increment_device");
    }

    /// What clean(victims) would move and need now: per victim batch its
    /// records and live objects, tombstones and entry bytes (d_usage,
    /// nullable), and the summary whose needed_bytes and needed_records size
    /// clean's outputs.  `victims` is a host array.  Changes nothing.
    void
    cleanSize(const uint32_t* victims, uint32_t nVictims, ramcrc_clean_usage* d_usage,
              ramcrc_clean_summary* d_summary, void* stream = NULL)
    {
        check(ramcrc_replay_table_clean_size_device(table, victims, nVictims, d_usage, d_summary,
                                                    stream),
              "ramcrc_replay_table_clean_size_device");
    }

    /// The log cleaner's relocation (LogCleaner::relocateLiveEntries,
    /// src/LogCleaner.cc:575-722, over ObjectManager::relocateObject and
    /// relocateTombstone) for the batches `victims` (a host array): the
    /// records the table still references are appended to d_out, byte for
    /// byte, and the table is re-pointed to them; everything else is dropped.
    /// d_out becomes the next batch without a walk and without an add():
    /// *d_outCert, *d_outStatus, d_outEntries, *d_outNEntries and d_outWork
    /// are written as certify, the walk and add() would write them, and stay
    /// the table's like an added batch's arrays.  d_moved[j] (nullable) is
    /// survivor j's old {batch, record}; its new one is {the returned number,
    /// j}.  Once `stream` has passed the call the victims' arrays are the
    /// caller's again.  Survivors that do not fit spoil the table: size the
    /// outputs with cleanSize().  Returns the survivor batch's number.
    uint32_t
    clean(const uint32_t* victims, uint32_t nVictims, void* d_out, uint32_t outCapacity,
          ramcrc_seg_cert* d_outCert, ramcrc_seg_status* d_outStatus,
          ramcrc_seg_entry* d_outEntries, uint64_t outEntriesCap, uint64_t* d_outNEntries,
          uint64_t* d_outWork, ramcrc_replay_ref* d_moved, ramcrc_clean_usage* d_usage,
          ramcrc_clean_summary* d_summary, void* stream = NULL)
    {
        uint32_t batch = 0;
        check(ramcrc_replay_table_clean_device(table, victims, nVictims, d_out, outCapacity,
                                               d_outCert, d_outStatus, d_outEntries, outEntriesCap,
                                               d_outNEntries, d_outWork, d_moved, d_usage,
                                               d_summary, &batch, stream),
              "ramcrc_replay_table_clean_device");
        return batch;
    }

    /// The source side of MasterService::migrateTablet
    /// (src/MasterService.cc:1084-1225, over migrateSingleLogEntry,
    /// :935-1073): the objects and tombstones of tableId whose key hash lies
    /// in [firstKeyHash, lastKeyHash], from the batches `batches` (a host
    /// array, in log order) starting at record startRecord of
    /// batches[startIndex], are packed as Segment::append packs them into up
    /// to maxSegments transfer segments of outCapacity bytes, output k at
    /// d_out + k * outStride, each sealed with d_outCerts[k]; d_outCounts[k]
    /// holds its entries.  flags: 0, or RAMCRC_MIGRATE_LIVE_ONLY to send only
    /// the records that are their key's winner now.  d_sent (nullable,
    /// sentCap entries) receives every sent entry's {batch, record},
    /// d_segFirst (nullable) the index of every output's first entry.
    /// d_summary carries the cursor for the next call (next_index,
    /// next_record), done and too_large.  The receiving side is a walk of the
    /// outputs under d_outCerts and an add() into the destination table.
    /// Read-only on the table.
    void
    migrateTablet(const uint32_t* batches, uint32_t nBatches, uint64_t tableId, uint64_t firstKeyHash,
                  uint64_t lastKeyHash, uint32_t flags, uint32_t startIndex, uint32_t startRecord,
                  void* d_out, uint32_t outCapacity, uint64_t outStride, uint32_t maxSegments,
                  ramcrc_seg_cert* d_outCerts, ramcrc_migrate_count* d_outCounts,
                  ramcrc_replay_ref* d_sent, uint64_t sentCap, uint64_t* d_segFirst,
                  ramcrc_migrate_summary* d_summary, void* stream = NULL)
    {
        check(ramcrc_replay_table_migrate_device(table, batches, nBatches, tableId, firstKeyHash,
                                                 lastKeyHash, flags, startIndex, startRecord, d_out,
                                                 outCapacity, outStride, maxSegments, d_outCerts,
                                                 d_outCounts, d_sent, sentCap, d_segFirst, d_summary,
                                                 stream),
              "ramcrc_replay_table_migrate_device");
    }

  private:
    static void
    check(int rc, const char* what)
    {
        if (rc != RAMCRC_OK)
            RAMCRC_BATCH_THROW(std::string(what) + ": " + ramcrc_strerror(rc));
    }

    ramcrc_replay_table* table;
    ramcrc_ctx* ctx;   // the batch's: an index lookup takes a context, not a table

    ReplayTable(const ReplayTable&);             // not copyable
    ReplayTable& operator=(const ReplayTable&);
};

/**
 * The recovery-scan batch sharded across the GPUs of a node (ramcrc_shard_*,
 * SURVEY.md 8(e)): every rank scans the contiguous range of replicas that
 * sits in its own HBM and one RCCL all-gather of the 4-byte results leaves
 * all CRCs, in segment order, with every rank -- what
 * BackupMasterRecovery::CyclicReplicaBuffer::buildNext
 * (src/BackupMasterRecovery.cc:743-809) checks per replica, for a whole
 * batch at once.  Errors throw like Crc32CBatch's.
 */
class Crc32CShard {
  public:
    /// One process driving several GPUs (ncclCommInitAll).
    explicit Crc32CShard(const std::vector<int>& devices)
        : shard(NULL)
    {
        check(ramcrc_shard_create_all(devices.empty() ? NULL : &devices[0],
                                      static_cast<int>(devices.size()), &shard),
              "ramcrc_shard_create_all");
    }

    /// One process per GPU (ncclCommInitRank); every process passes the same
    /// uniqueId() bytes, produced by one of them.
    Crc32CShard(const std::vector<uint8_t>& id, int nranks, int rank, int device)
        : shard(NULL)
    {
        if (id.size() != RAMCRC_SHARD_ID_BYTES)
            RAMCRC_BATCH_THROW(std::string("Crc32CShard: unique id must be 128 bytes"));
        check(ramcrc_shard_create_rank(&id[0], nranks, rank, device, &shard),
              "ramcrc_shard_create_rank");
    }

    ~Crc32CShard()
    {
        if (shard)
            ramcrc_shard_destroy(shard);
    }

    static std::vector<uint8_t>
    uniqueId()
    {
        std::vector<uint8_t> id(RAMCRC_SHARD_ID_BYTES);
        check(ramcrc_shard_unique_id(&id[0]), "ramcrc_shard_unique_id");
        return id;
    }

    /// [first, last) of the segments rank `rank` of `nranks` owns.
    static std::pair<uint64_t, uint64_t>
    range(uint64_t segments, int nranks, int rank)
    {
        uint64_t lo = 0, hi = 0;
        check(ramcrc_shard_range(segments, nranks, rank, &lo, &hi), "ramcrc_shard_range");
        return std::make_pair(lo, hi);
    }

    /**
     * One recovery-scan step: dShard[k] (device memory of local rank k)
     * holds that rank's range() of `segments` replicas of segmentBytes each.
     * Returns the finalized CRCs of all segments, in segment order, as
     * gathered on local rank 0.  Synchronous.
     */
    std::vector<uint32_t>
    deviceShard(const std::vector<const void*>& dShard, uint64_t segmentBytes,
                uint64_t segments)
    {
        if (static_cast<int>(dShard.size()) != ramcrc_shard_local_count(shard))
            RAMCRC_BATCH_THROW(std::string("Crc32CShard: one buffer per local rank"));
        std::vector<uint32_t> out(segments);
        check(ramcrc_shard_segments(shard, dShard.empty() ? NULL : &dShard[0], segmentBytes,
                                    segments, NULL, RAMCRC_FINALIZE),
              "ramcrc_shard_segments");
        check(ramcrc_shard_sync(shard), "ramcrc_shard_sync");
        if (segments)
            check(ramcrc_shard_results(shard, 0, &out[0], segments), "ramcrc_shard_results");
        return out;
    }

  private:
    static void
    check(int rc, const char* what)
    {
        if (rc != RAMCRC_OK)
            RAMCRC_BATCH_THROW(std::string(what) + ": " + ramcrc_strerror(rc));
    }

    ramcrc_shard* shard;

    Crc32CShard(const Crc32CShard&);             // not copyable
    Crc32CShard& operator=(const Crc32CShard&);
};

} // namespace RAMCloud

#endif // RAMCLOUD_CRC32CBATCH_H
