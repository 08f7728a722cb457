/*
 * kasa_hip.h -- C ABI of the MI355X (gfx950) implementation of kASA's `identify` hot path.
 *
 * kASA has no plugin/FFI interface: the hot path is the set of calls that
 * Compare::CompareWithLib_partialSort (source/modes/Compare.hpp:2733) makes per batch.  This header
 * declares exactly those calls as a drop-in seam; each entry names the reference code it replaces.
 * Plain pointers and sizes only; every buffer passed in is owned by the caller and only borrowed for
 * the duration of the call; nothing returned outlives kasa_ctx_destroy / kasa_index_destroy.
 *
 * Errors: the reference throws std::runtime_error / bad_alloc and prints "ERROR: <what>"
 * (source/main.cpp:1717-1720).  Here every call returns a status (0 = ok) and never lets a C++
 * exception or HIP error cross the boundary; kasa_last_error() returns the message the host wrapper
 * rethrows as runtime_error (INTEGRATION.md shows the reference-side binding).
 *
 * Threading (Compare.hpp:3263-3283, main.cpp:1292-1326): a kasa_index is immutable after creation
 * and may be shared by any number of contexts / threads; a kasa_ctx (stream, batch buffers, profile
 * tables) is single-threaded.
 *
 * Table layout everywhere: [level * nTaxa + taxIdx], level 0 = kHigh ... nK-1 = kLow, taxIdx = dense
 * index of the content file (0 = "non_unique"), exactly Compare.hpp:922.
 */
#ifndef KASA_HIP_H
#define KASA_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kasa_index kasa_index;
typedef struct kasa_ctx kasa_ctx;

enum {
    KASA_OK = 0,
    KASA_E_ARG = 1,       /* bad argument (the message says which) */
    KASA_E_HIP = 2,       /* a HIP runtime call failed */
    KASA_E_NOMEM = 3,     /* device or host allocation failed (reference: bad_alloc) */
    KASA_E_STATE = 4,     /* calls out of order (e.g. lookup before sort) */
    KASA_E_LIMIT = 5      /* a documented capacity limit was hit (message says which) */
};

/* stages of one batch, for kasa_ctx_stage_ms() */
enum {
    KASA_STAGE_ENCODE = 0,   /* Read.hpp:763-827  convertAndSort -> convertLinesTokMers_new */
    KASA_STAGE_SORT = 1,     /* Compare.hpp:1077/1130 sort by k-mer */
    KASA_STAGE_LOOKUP = 2,   /* Compare.hpp:1098-1117 + :803-829,:861-995: prefix table + search */
    KASA_STAGE_GROUP = 3,    /* Compare.hpp:917-955,1005-1041: per-level groups, taxon sets, flush order */
    KASA_STAGE_REGROUP = 4,  /* slots of the queries in read order when the encoder could not rank them (stable sort by read) */
    KASA_STAGE_SCORE = 5,    /* Compare.hpp:516-532 score accumulation in reference order */
    KASA_STAGE_COUNT = 6
};

/* Message of the last failed call on this thread ("" if none). */
const char *kasa_last_error(void);

/* Number of visible HIP devices (0 if none / no driver). */
int kasa_device_count(int *count);

/* ---- index residency: replaces Compare::ReadIndex::loadIndex / loadTrie / loadContentAndFrequencyFiles
 *      (source/modes/Compare.hpp:111-337).
 * records   : nRecords packed {u64 kmer, u32 taxid} entries of 12 bytes, sorted by (kmer, taxid) --
 *             the index file as it is on disk (may be an mmap of it); or, with recordBytes = 6, the
 *             "halved" index of shrink strategy 2, {u32 low 30 bits, u16 dense taxon index}
 *             (source/utils/packedPairs.hpp:100-105), which needs the trie arrays; or, with
 *             recordBytes = 20, the 128-bit index of `build --kH 25`: {u64 low, u64 high, u32 taxid}
 *             (packedLargePair, packedPairs.hpp:132-155; _info.txt carries the marker 128), 25 letters
 *             per k-mer, levels up to k = 25.
 * triePrefix/trieCount : the `_trie` file (source/modes/Trie.hpp:365-394): 30-bit prefixes ascending
 *             and their entry counts; may be NULL/0 -- the device derives its own two-level prefix
 *             table from the records and, when given, checks it against this one.
 * taxIds    : taxIds[i] = tax ID of dense index i as in the content file (taxIds[0] = 0), nTaxa
 *             entries (Compare.hpp:121-151).
 */
int kasa_index_create(int device, const void *records, uint64_t nRecords, int recordBytes,
                      const uint32_t *triePrefix, const uint64_t *trieCount, uint64_t nTrie,
                      const uint32_t *taxIds, uint32_t nTaxa, kasa_index **out);
void kasa_index_destroy(kasa_index *ix);
uint64_t kasa_index_size(const kasa_index *ix);
uint64_t kasa_index_device_bytes(const kasa_index *ix);

/* ---- context: replaces the kASA / Read / Compare constructors (source/kASA.hpp:276-305) and
 *      setCodonTable (source/kASA.hpp:579-615).
 * kHigh/kLow : -k <kHigh> <kLow>, at most 12 with a 64-bit index and 25 with a 128-bit one; frames: 3 (default), 6 (--six) or 1 (--one, Read.hpp:223-261);
 * codonLut: 366-byte table of 5-bit letter codes indexed like kASA.hpp:75, or NULL for the built-in
 * table (kASA.hpp:621-667).
 */
int kasa_ctx_create(const kasa_index *ix, int kHigh, int kLow, int frames, const uint8_t *codonLut,
                    kasa_ctx **out);
/* The built-in table (kASA.hpp:621-667) in the codonLut layout: the starting point for -a/--alphabet, which
 * overwrites the 64 codons of an NCBI gc.prt table in it (kASA::setCodonTable, kASA.hpp:579-615).  Host only. */
int kasa_builtin_codon_table(uint8_t *lut366);
void kasa_ctx_destroy(kasa_ctx *ctx);

/* The next batches hold amino-acid sequences instead of DNA (what kASA::detectAlphabet decides per
 * input file, kASA.hpp:155-183): letters are taken as they are ('*' -> '[', code = char & 31), padding
 * and marker are '^', a read of L letters gives L-K+1 k-mers (Read.hpp:36-41,60-81,636-640,663-667,
 * 1069-1073); --six is switched off (kASA.hpp:181).  protein = 0 returns to DNA. */
int kasa_ctx_set_protein(kasa_ctx *ctx, int protein);

/* ---- one batch ------------------------------------------------------------------------------- */

/* Hand the raw reads of one batch to the device: concatenated bases and offsets[nReads+1].
 * Replaces the vLines the reference keeps per batch (Read.hpp:612-630).  Cleaning (non-ACGT -> Z),
 * padding and the X marker (Read.hpp:633-675,1068-1078) happen on the device.  One copy only; `bases` may also point into
 * device memory (a host that keeps the reads of a whole file resident, as bench.py does for its multi-batch steps);
 * `offsets` is host memory. */
int kasa_batch_upload(kasa_ctx *ctx, const uint8_t *bases, const int64_t *offsets, int64_t nReads);

/* The same for a host that keeps the reads of a whole file resident in HBM (bench.py's steps at every N, a pipeline that
 * parses on the device): `basesDev` AND `offsetsDev` (int64[nReads+1], relative to basesDev) lie in device memory.  Nothing
 * crosses PCIe and the bases are NOT copied: the context reads them in place, so they must stay valid and unchanged until
 * the batch's last call (kasa_batch_coherence re-reads them).  What is left of the upload is the geometry of Read.hpp:36-57,
 * 633-675 on the device (k-mers per read, running sums) and one 8-byte read-back of the batch's k-mer count.  A host
 * that parses on the device gets such reads from kasa_parse_append and hands them on with kasa_parse_take (below). */
int kasa_batch_upload_device(kasa_ctx *ctx, const uint8_t *basesDev, const int64_t *offsetsDev, int64_t nReads);

/* The same for reads made of several sequences: paired-end input (-1/-2; Read::readFastqa_pairedEnd,
 * Read.hpp:834-1049) hands both mates of a pair on as two entries of vLines with ONE read id, so their
 * k-mers score into the same row and none spans the junction.  offsets[nSegments+1] delimit the
 * sequences, segmentRead[s] (ascending, < nReads) names the read of sequence s. */
int kasa_batch_upload_segments(kasa_ctx *ctx, const uint8_t *bases, const int64_t *offsets, int64_t nSegments,
                               const uint32_t *segmentRead, int64_t nReads);

/* Read::convertAndSort (Read.hpp:763-827): every read -> packed k-mers + read id, device resident. */
int kasa_batch_encode(kasa_ctx *ctx, uint64_t *nKmers);
/* Reads a wavefront of the encoder takes together when a batch is DNA in three frames with at most 192 k-mers per read
 * (the group form of the encoder; every other batch: one read per wavefront). */
int kasa_encode_group_reads(void);

/* Compare::sortInputAndCheckInvalidkMers_sta (Compare.hpp:1074-1260): sort by k-mer and find each
 * query's place in the index.  unique != 0 is -e/--unique (Compare.hpp:3167-3178): records equal in
 * (k-mer, read id) are kept once.  The reference applies std::unique to an unstable sort, so duplicates
 * it happens not to place side by side survive there; here all of them are dropped. */
int kasa_batch_sort_and_range(kasa_ctx *ctx, int unique);

/* Compare::compareWithDatabase + scoreMatchForReadIDsAndTaxIDs (Compare.hpp:678-1069,516-673):
 * adds this batch into the context's profile tables; with wantPerRead also produces the non-zero
 * cells of the reads x taxa score matrix (Utilities.hpp:592-636) as a CSR. */
int kasa_batch_lookup_score(kasa_ctx *ctx, int wantPerRead, int coverage);

/* The two halves of kasa_batch_lookup_score as separate steps, with the event records in between exposed, for an index
 * that is range-partitioned over devices (C5; the reference's loadIndex has no such mode, the seam is ours):
 *   kasa_batch_group          one record per sorted query, in sorted order: 8 (up to 8 levels) or 16 (up to 25 levels)
 *                             32-bit words {position, last flush position, deepest level | flush order of its events |
 *                             flags, number of taxon segments | sizes of the taxon sets per level (narrow records),
 *                             [wide: the flush order, 4 words], up to 4 (8) segments -- or 3 (7) and the pool offset of a
 *                             longer list: pool block = {number of segments, [4 words of exact set sizes when the
 *                             record's "crowded" flag is set], the further segments}};
 *                             a segment = taxon | first level << 22 | last level << 27, so an index may name at most
 *                             2^22 taxa (layout: kasa_amd/csrc/kasa_hip.hip "event records", DESIGN.md sections 3-4).
 *                             Records and pools are opaque to a caller that only moves them; they are NOT a stable
 *                             format across versions of this library;
 *   kasa_batch_records_*      size (in 32-bit words) / download of records and pool; import hands records in sorted order
 *                             to a context whose batch is sorted, which files them by read;
 *   kasa_batch_score          replays the records per read (scores, profile) exactly as kasa_batch_lookup_score does. */
int kasa_batch_group(kasa_ctx *ctx, int coverage);
/* kasa_batch_group with the records written straight into the caller's device buffer (room for
 * number of queries x record words u32): the partition worker groups a slice into the tensor its collective sends, no copy
 * in between.  kasa_batch_records_device then reports that pointer; the pool stays the context's. */
/* (recordsOutDev must lie on the context's device -- group_kernel stores into it: KASA_E_ARG names the two devices otherwise) */
int kasa_batch_group_to(kasa_ctx *ctx, int coverage, uint32_t *recordsOutDev);
int kasa_batch_score(kasa_ctx *ctx, int wantPerRead);
int kasa_batch_records_size(kasa_ctx *ctx, uint64_t *nRecordWords, uint64_t *nPoolWords);
int kasa_batch_records_fetch(kasa_ctx *ctx, uint32_t *records, uint32_t *pool);
int kasa_batch_records_import(kasa_ctx *ctx, const uint32_t *records, uint64_t nRecordWords, const uint32_t *pool, uint64_t nPoolWords);

/* The same exchange without the host: slices of the sorted queries and the records made from
 * them are handed over as DEVICE pointers, so the caller's collective (RCCL all_to_all over xGMI) moves them from HBM to
 * HBM.  Pointers returned by the *_device getters point into the context's own buffers and stay valid until its next
 * batch call.  Pointers passed in may lie on ANY device of the process: what they name is copied to (or from) a buffer on the
 * context's own device before (after) a kernel works on it, so no kernel ever touches another device's memory and peer access
 * is neither needed nor enabled.  The few calls whose kernels work in the caller's buffer itself (kasa_batch_group_to,
 * kasa_batch_records_pack_size / _pack / _unpack, kasa_batch_upload_device) return KASA_E_ARG, naming both devices, for a
 * buffer that lies elsewhere.
 *   kasa_batch_queries_device         the sorted k-mers of the batch (8 or 16 bytes each) and their number
 *   kasa_batch_slice_starts           starts[j] = first sorted query whose 30-bit prefix is >= cuts[j] (starts[0] = 0,
 *                                     starts[nParts] = number of queries): slice j goes to the owner of partition j
 *   kasa_batch_set_sorted_device      installs a slice of sorted k-mers as a batch of its own and looks it up
 *                                     (kasa_batch_set_queries + kasa_batch_sort_and_range without the sort);
 *                                     kasa_batch_group then makes its records
 *   kasa_batch_records_device         records (sorted order) and pool of the grouped slice
 *   kasa_batch_records_import_device  the slices' records, in partition order, become the batch's records: positions
 *                                     move by the slice starts and pool offsets by the pool bases on the device
 *                                     (what kasa_amd/partition.py:assemble_records does for the host path); records that
 *                                     are not in their place of the inbox yet are copied there first, pools are copied */
int kasa_batch_queries_device(kasa_ctx *ctx, const void **kmers, uint64_t *n);
int kasa_batch_slice_starts(kasa_ctx *ctx, const uint64_t *cuts, uint32_t nParts, uint64_t *starts);
int kasa_batch_set_sorted_device(kasa_ctx *ctx, const void *kmersDev, uint64_t n);
int kasa_batch_records_device(kasa_ctx *ctx, const uint32_t **records, uint64_t *nRecordWords, const uint32_t **pool, uint64_t *nPoolWords);
int kasa_batch_records_import_device(kasa_ctx *ctx, uint32_t nParts, const uint32_t *const *records, const uint64_t *nRecordWords,
                                     const uint32_t *const *pool, const uint64_t *nPoolWords);
/* The staging buffer kasa_batch_records_import_device files the records from, with room for nRecordWords words: a caller that
 * receives the slices' records THERE (back to back, in partition order) and names those places as `records[j]` spares the
 * batch a second copy of its records (32 or 64 bytes per query); they are then shifted in place. */
int kasa_batch_records_inbox(kasa_ctx *ctx, uint64_t nRecordWords, uint32_t **records);
/* The records of an exported slice PACKED for the wire (the return leg of the partitioned exchange; ours -- the reference streams
 * its index from disk and exchanges nothing): one byte of classes per four records (2 bits each: unmatched / words [1..4] /
 * [1..6] / [1..7] of a 32-byte record, [1..9] / [1..11] / [1..15] of a 64-byte one, by its number of segments), padded to 16
 * bytes, then those words back to back; word [0] -- the query's place in the slice -- is implied.  SURVEY 8(e) sizes the
 * exchange at 12-20 bytes per query.  pack_size (one pass over the records: the sizes) then pack, on the context that grouped
 * the slice (records = what kasa_batch_group_to / kasa_batch_records_device gave); unpack on the read owner, into the place
 * the whole records would have been received at (kasa_batch_records_inbox), before kasa_batch_records_import_device. */
int kasa_batch_records_pack_size(kasa_ctx *ctx, const uint32_t *recordsDev, uint64_t nQueries, uint64_t *nBytes);
int kasa_batch_records_pack(kasa_ctx *ctx, const uint32_t *recordsDev, uint64_t nQueries, void *outDev, uint64_t capBytes);
int kasa_batch_records_unpack(kasa_ctx *ctx, const void *packedDev, uint64_t nBytes, uint64_t nQueries, uint32_t *recordsOutDev);


/* CSR of the batch: readOffsets[nReads+1]; per read taxIdx ascending with score > 0 -- the cells
 * scoringFunc scans (Compare.hpp:1501-1522). */
int kasa_batch_scores_size(kasa_ctx *ctx, uint64_t *nnz);
int kasa_batch_scores_fetch(kasa_ctx *ctx, uint64_t *readOffsets, uint32_t *taxIdx, float *score);

/* --coherence (Compare::postProcess, Compare.hpp:2607-2728, fed by setMatchLength at :847-848,882-884,912-914,948; printed at
 * :1662-1665 and used by --filter at :1602-1606).  Per read the reference's coherence score of
 * the batch that was last sorted (kasa_batch_sort_and_range): the k-mers in the order the reader emitted them (read, strand,
 * window), match length = the deepest matched level of the k-mer, clusters of overlapping matches walked with the
 * reference's own state machine -- including what it credits to reads without k-mers and what it skips after a strand
 * switch.  scores = float[nReads] (host).  *throwsAt = ~0, or the index at which the reference's walk runs off the end of
 * its vector (std::out_of_range from vector::at, Compare.hpp:2667: with --six, a batch whose last strand switch finds no
 * further match): then the reference ends with "vector::_M_range_check: __n (which is N) >= this->size() (which is N)",
 * N = *throwsAt, and the host should do the same.  Single-end batches without -e only (the reference's results for the
 * others depend on its unstable sorts): KASA_E_ARG otherwise. */
int kasa_batch_coherence(kasa_ctx *ctx, float *scores, uint64_t *throwsAt);

/* The same over a range-partitioned index (C5; the reference streams an index of any size through the same walk,
 * Compare.hpp:182-328, so the seam is ours): kasa_batch_coherence cut at the one step that reads the index.  A k-mer's match
 * length (setMatchLength, Compare.hpp:847-848,882-884,912-914,948) needs at least the 6 letters of a `_trie` entry
 * (Trie.hpp:494-520) in common with an index entry, and partitions are cut between `_trie` entries: its depth against the
 * whole index is its depth against the partition that owns its 30-bit prefix, and 0 against every other one.
 *   kasa_batch_coherence_begin     on the context that owns the reads, after kasa_batch_score: the preconditions and errors
 *                                  of kasa_batch_coherence; encodes the batch once more in emission order (read, strand,
 *                                  window; Compare.hpp:2609-2628 sorts it back into that order) and hands out the k-mers
 *                                  (8 or 16 bytes each), their number *n (what kasa_batch_encode reported) and *n depth
 *                                  bytes, all zero.  The pointers stay valid until the context's next batch call.
 *   kasa_batch_match_depth_device  on a context bound to ONE partition (or to the whole index: [0, 2^30)): for every k-mer
 *                                  whose 6-letter prefix p satisfies firstPrefix <= p < endPrefix -- the units of
 *                                  kasa_batch_slice_starts' `cuts`; 2^30 ends the last partition -- depthDev[i] = the deepest
 *                                  level of k-mer i that this context's index matches, by this context's -k (at least 6
 *                                  letters, cut before the first '^', 0 below the lowest level: Compare.hpp:803-829,847-948).
 *                                  K-mers of other prefixes are skipped before the index is touched and their bytes are
 *                                  left as they are.  kmersDev and depthDev may lie on any device; the batch this
 *                                  context holds is not disturbed.  n must be the n of _begin.
 *   kasa_batch_coherence_finish    on the owner, once every partition has had its call: finds the first matching k-mer
 *                                  (Compare.hpp:2630-2646) from the depth bytes and walks them (Compare.hpp:2663-2728);
 *                                  scores, *throwsAt and the effect on kasa_batch_text as kasa_batch_coherence.
 * kmersDev and depthDev are copied to the partition's device and the bytes back (no kernel of `part` reads or writes them in
 * place), so they may lie anywhere.  With the partitions on several devices the same step in two halves, one per device:
 *   kasa_batch_match_depth_stage   on the partition context: copies the n k-mers to its own device, zeroes n depth bytes of its
 *                                  own, runs the same kernel over [firstPrefix, endPrefix) and hands those bytes out
 *                                  (*depthDev: valid until the context's next depth call; a byte is non-zero only where this
 *                                  partition gave a depth).  Arguments and errors as kasa_batch_match_depth_device.
 *   kasa_batch_coherence_fold      on the owner, between _begin and _finish: copies such bytes to its device and takes the
 *                                  bytewise maximum with the batch's depth bytes.  A k-mer has a depth in at most one
 *                                  partition, so after one fold per partition the bytes are what one
 *                                  kasa_batch_match_depth_device per partition leaves.  n must be the n of _begin.
 *                                  Stages of different partition contexts may run at the same time (one host thread
 *                                  each); the folds are the owner's calls, one after the other.
 * Each call returns with its stream idle, so a host needs no synchronisation of its own between contexts.  KASA_E_STATE:
 * _finish or _fold without _begin on this batch; KASA_E_ARG: firstPrefix > endPrefix or beyond 2^30, an n that is not the batch's. */
int kasa_batch_coherence_begin(kasa_ctx *owner, const void **kmersDev, uint64_t *n, uint8_t **depthDev);
int kasa_batch_match_depth_device(kasa_ctx *part, uint64_t firstPrefix, uint64_t endPrefix, const void *kmersDev, uint64_t n, uint8_t *depthDev);
int kasa_batch_match_depth_stage(kasa_ctx *part, uint64_t firstPrefix, uint64_t endPrefix, const void *kmersDev, uint64_t n, const uint8_t **depthDev);
int kasa_batch_coherence_fold(kasa_ctx *owner, const uint8_t *depthDev, uint64_t n);
int kasa_batch_coherence_finish(kasa_ctx *owner, float *scores, uint64_t *throwsAt);

/* Ranking on the device (Compare::scoringFunc, Compare.hpp:1495-1594 and the printing loops
 * :1721-1754): instead of the whole CSR only what the per-read file can print leaves the device.
 *   den        [nClasses][nTaxa] doubles, row c = 1 + log2(freq[t] * double(uint32(len_c - 3K + 1))) for the c-th distinct
 *              read length of the batch (len_c - K + 1 for protein input), computed by the host with libm exactly as
 *              Compare.hpp:1506-1511 does; readClass[r] = the row of read r
 *   threshold  -t (relative scores below it are dropped), beasts = -b
 * Per read the hits are taken in the order (relative score descending, taxon ascending) for as long as the TSV or the
 * JSON / JSONL / Kraken writer would print another one.  kasa_batch_rank_fetch delivers
 *   meta[4 r .. 4 r + 3] = { first entry, number of entries | flag << 31, float bits of the largest k-mer score among
 *                            the hits, number of hits }
 *   entries[i]           = { uint32 taxIdx, float kmerScore, double relativeScore }   (16 bytes)
 * (nEntries = length of the entries array; reads own disjoint ranges of it, handed out in slabs, so some entries
 * between them are unused)
 * A writer that runs the reference's loops over these entries (as if they were all hits, with the delivered maximum)
 * prints what it would print from the full row.  Where more than 16 hits meet a tie in the relative score inside the
 * printed prefix, the order is std::sort's own (not stable, but deterministic): those reads are ranked by a second kernel
 * that walks libstdc++'s introsort over the hits (kasa_amd/csrc/stdsort_order.h).  flag: the read could not be ranked on
 * the device (std::sort would have switched to its heap sort, or the row has 65 536 or more cells): it gets no entries
 * and the host ranks it from its full row (kasa_batch_scores_fetch).  nFlagged counts such reads.
 * The call may use the batch's event records as scratch: kasa_batch_group has to run again before another kasa_batch_score
 * of the same batch (the scores themselves, kasa_batch_scores_fetch, stay valid). */
int kasa_batch_rank(kasa_ctx *ctx, const double *den, uint32_t nClasses, const uint32_t *readClass, float threshold, uint32_t beasts,
                    uint64_t *nEntries, uint32_t *nFlagged);
int kasa_batch_rank_fetch(kasa_ctx *ctx, uint32_t *meta, void *entries);

/* The per-read file's text written on the device (the printing loops of Compare::scoringFunc,
 * Compare.hpp:1526-1872, with the reference's number formats utils/iToStr.hpp:35-114 and utils/dToStr.h:427-456): after
 * kasa_batch_rank the hits never leave the device -- a kernel writes every read's TSV / JSON / JSON-lines / Kraken bytes
 * into one buffer (read order, offsets by a prefix sum of the sizes), and what crosses PCIe is the next piece of the file.
 *   kasa_ctx_set_taxa_text  once per context: taxIds[nTaxa] and the names of the content file (entry 0 = "non_unique"),
 *                           back to back, names[nameOff[t] .. nameOff[t+1])
 *   kasa_batch_text         the text of the batch last ranked.  KASA_E_STATE when kasa_batch_rank left reads to the host
 *                           (nFlagged > 0: the host then writes the whole batch from kasa_batch_rank_fetch +
 *                           kasa_batch_scores_fetch as before)
 *   kasa_batch_text_fetch   text[nBytes] (NULL: the text stays where it is, see kasa_batch_text_fetch_range); readOffsets[nReads + 1]
 *                           (may be NULL): where each read's text starts;
 *                           contaminated[nReads] (may be NULL): 1 = --filter's rule holds for the read (Compare.hpp:1597-1606:
 *                           within errorThreshold of the perfect score, or coherence >= coherenceThreshold) */
enum { KASA_TEXT_TSV = 0, KASA_TEXT_JSON = 1, KASA_TEXT_JSONL = 2, KASA_TEXT_KRAKEN = 3 };
typedef struct kasa_text_params {
    int format;                    /* KASA_TEXT_* */
    uint32_t beasts;               /* -b */
    uint64_t firstRead;            /* number of the batch's first read in its file ("Read number") */
    const char *readNames;         /* host: the specifiers as printed, back to back */
    const uint64_t *readNameOff;   /* host: [nReads + 1] */
    const uint32_t *readLen;       /* host: "Length" of every read */
    const float *bestScore;        /* host: [nClasses] the perfect score of a read of class c (Compare.hpp:1452-1481); classes =
                                      the readClass given to kasa_batch_rank */
    uint32_t nClasses;
    int coherence;                 /* print the coherence of the read (the scores of kasa_batch_coherence on this batch) */
    double errorThreshold;         /* --errorThreshold, as a double */
    float coherenceThreshold;      /* --coherenceThreshold */
} kasa_text_params;
int kasa_ctx_set_taxa_text(kasa_ctx *ctx, const uint32_t *taxIds, const char *names, const uint64_t *nameOff);
int kasa_batch_text(kasa_ctx *ctx, const kasa_text_params *params, uint64_t *nBytes);
int kasa_batch_text_fetch(kasa_ctx *ctx, char *text, uint64_t *readOffsets, uint8_t *contaminated);
/* text[offset .. offset + nBytes) of the same text: a host that moves it through a few small page-locked buffers (making one
 * of 5.5 GB for the text of 10 M reads takes seconds) writes one piece to the file while the next one arrives. */
int kasa_batch_text_fetch_range(kasa_ctx *ctx, char *text, uint64_t offset, uint64_t nBytes);
/* Test tap: the reference's double -> text (dToStr.h) as the device writes it; out = 32 bytes per value, zero-terminated. */
int kasa_text_dtoa(int device, const double *values, uint32_t n, char *out);

/* The same text compressed on the device (ours: the reference's --gzip covers the --filter files only): a BGZF stream, the
 * blocked gzip of htslib / bgzip that gzip -d, zcat and every gzip reader take.  Block i covers the text's bytes
 * [i 65280, (i + 1) 65280) and is one complete gzip member: header 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, the subfield
 * 'B' 'C' 02 00 BSIZE (member length - 1), one raw deflate stream with BFINAL = 1 in RFC 1951's fixed Huffman code -- or
 * stored, when that is not smaller -- then CRC-32 and ISIZE.  A member has at most 65536 bytes; the same text gives the same
 * bytes on every run.  The stream has NO end-of-file block (28 bytes, the same for every file): whoever closes the file
 * appends it.  The text itself stays where it is: kasa_batch_text_fetch* deliver it afterwards as before.
 *   kasa_batch_bgzf              after kasa_batch_text: the same text as a BGZF stream; *nBytes its length, *nBlocks its members
 *                                (an empty text: 0 and 0).  KASA_E_STATE without a text of this batch.
 *   kasa_batch_bgzf_fetch_range  dst[nBytes] = stream[offset .. offset + nBytes): any offset, any length inside the stream
 *                                (pieces need not end with a member).  KASA_E_STATE without a stream of this batch's text. */
int kasa_batch_bgzf(kasa_ctx *ctx, uint64_t *nBytes, uint64_t *nBlocks);
int kasa_batch_bgzf_fetch_range(kasa_ctx *ctx, void *dst, uint64_t offset, uint64_t nBytes);
/* Test tap (like kasa_text_dtoa): n host bytes through the same kernels; *nOut = stream length, KASA_E_LIMIT when dstCap is too small. */
int kasa_bgzf_deflate(int device, const void *src, uint64_t n, void *dst, uint64_t dstCap, uint64_t *nOut);
/* The code of the members' deflate streams.  KASA_BGZF_DYNAMIC: ONE Huffman table per stream (per kasa_batch_bgzf call), made
 * on the device from the symbols of a sample of the text's blocks (all of them up to 64, else blocks floor(j nBlocks / 64),
 * j = 0..63; every symbol keeps a code, of 15 bits at most), and written into every member: BTYPE = 10, HLIT = 29, HDIST = 29,
 * a complete fixed code-length code without run-length symbols.  The matcher and the tokens are the fixed code's; a member is
 * still written stored when its coded form is not smaller, and a block of fewer than 2048 bytes keeps the fixed code (a table's
 * header costs what it saves there).  Bytes are as reproducible as before.
 *   kasa_ctx_set_bgzf_code    what the context's following kasa_batch_bgzf calls use; a context starts with KASA_BGZF_FIXED.
 *                             KASA_E_ARG for any other value (the context keeps its code).
 *   kasa_bgzf_deflate_coded   kasa_bgzf_deflate with a code; kasa_bgzf_deflate is KASA_BGZF_FIXED. */
enum { KASA_BGZF_FIXED = 0, KASA_BGZF_DYNAMIC = 1 };
int kasa_ctx_set_bgzf_code(kasa_ctx *ctx, int code);
int kasa_bgzf_deflate_coded(int device, int code, const void *src, uint64_t n, void *dst, uint64_t dstCap, uint64_t *nOut);

/* ---- BGZF in: members inflated on the device (ours: the reference reads .gz through zlib on one thread) -----------------
 * A BGZF file is tens of thousands of deflate streams (RFC 1951: stored, fixed and dynamic blocks, any number per member)
 * that state their own length (BSIZE) and content (ISIZE <= 65536): the host walks the headers, member i's text goes to the
 * running sum of ISIZE before it, one wavefront inflates one member and checks its CRC-32 (kasa_amd/csrc/kasa_inflate.h).
 * Gzip without the 'BC' subfield is one long stream and is not taken.  A malformed member is a STATUS, never a fault: every
 * load stays inside the member's payload, every store inside its ISIZE bytes, no back-reference reaches below its first byte.
 *   kasa_bgzf_inflate   test tap that mirrors kasa_bgzf_deflate: nBytes of host stream -> host text.  *nText = the ISIZE sum
 *                       of the stream's whole members; KASA_E_LIMIT (nothing written) when cap is smaller.  A bad stream:
 *                       KASA_OK with *status = the KASA_INFLATE_* code of the FIRST offending member and *member its index
 *                       (for KASA_INFLATE_HEADER / _CUT: the number of whole members before the bytes that are none); the
 *                       text is then not written.
 *   kasa_inflate_status_text  names a code. */
enum {
    KASA_INFLATE_OK = 0,
    KASA_INFLATE_HEADER = 1,        /* no BGZF member header (1f 8b 08 04 .. 06 00 'B' 'C' 02 00), BSIZE below 25 or ISIZE above 65536 */
    KASA_INFLATE_CUT = 2,           /* the stream ends inside a member */
    KASA_INFLATE_TRUNCATED = 3,     /* the deflate data end before the last block does */
    KASA_INFLATE_BTYPE = 4,         /* block type 3 */
    KASA_INFLATE_STORED_LEN = 5,    /* a stored block whose LEN is not the complement of NLEN */
    KASA_INFLATE_CODE_LENGTHS = 6,  /* a dynamic block's header: more than 286 / 30 codes stated, a repeat with no length before it or
                                       past the last one, a set that is over-subscribed or incomplete (but for a single one-bit
                                       code; the code-length code has to be complete), no end-of-block code */
    KASA_INFLATE_SYMBOL = 7,        /* a bit pattern that is no code, or a length / distance symbol outside the alphabet */
    KASA_INFLATE_DISTANCE = 8,      /* a back-reference to before the member's first byte */
    KASA_INFLATE_OVERRUN = 9,       /* more output than ISIZE states */
    KASA_INFLATE_SHORT = 10,        /* less output than ISIZE states */
    KASA_INFLATE_TRAILING = 11,     /* bytes between the last block and the trailer */
    KASA_INFLATE_CRC = 12,          /* the output's CRC-32 is not the trailer's */
    KASA_INFLATE_GZIP_HEADER = 13,  /* kasa_gzip_inflate: no gzip member header (1f 8b 08, no reserved flag) where one has to be */
    KASA_INFLATE_SPAN = 14          /* kasa_gzip_inflate: a block (one wavefront's text) longer than the span limit of 2^30 bytes */
};
int kasa_bgzf_inflate(int device, const void *stream, uint64_t nBytes, void *text, uint64_t cap, uint64_t *nText, int *status, uint64_t *member);
const char *kasa_inflate_status_text(int code);

/* ---- plain gzip in: ONE LONG deflate stream inflated on the device (ours; kasa_amd/csrc/kasa_gunzip.h) ------
 * The file gzip and pigz write has no member table, so the stream is cut into chunks of chunkBytes compressed bytes: every
 * chunk searches its own bits for a dynamic block header that validates, a wavefront per chunk decodes whole blocks from
 * there into 16-bit symbols (a byte, or a marker for a byte of the 32 KiB before the chunk), the host confirms the chain of
 * block boundaries round by round, and the markers are replaced once the windows are known.  The host parses the member
 * headers (FEXTRA, FNAME, FCOMMENT, FHCRC) and compares CRC-32 and ISIZE with each trailer; members follow one another.
 * The same contract as kasa_bgzf_inflate: a malformed stream is a status, never a fault and never a hang.
 *   kasa_gzip_inflate   test tap, host to host.  chunkBytes: 0 for the default (64 KiB), else 64 or more.  *nText = the text
 *                       of all members; KASA_E_LIMIT (nothing written) when cap is smaller.  A bad stream: KASA_OK with
 *                       *status = a KASA_INFLATE_* code and *member = the index of the member it is in (for
 *                       KASA_INFLATE_GZIP_HEADER: of the member that should begin there); the text is then not written.
 *                       ISIZE: a text shorter than stated is KASA_INFLATE_SHORT, a longer one KASA_INFLATE_OVERRUN.
 *                       stats8, when not NULL: chunks, chunks with a start (the first chunk of a member has one by
 *                       definition), chunks confirmed, candidates the chain rejected, rounds (the most any member took),
 *                       marker symbols written, capacity reruns, members.  Streams of 2 GiB and more are KASA_E_LIMIT. */
int kasa_gzip_inflate(int device, const void *stream, uint64_t nBytes, uint32_t chunkBytes, void *text, uint64_t cap, uint64_t *nText, int *status,
                      uint64_t *member, uint64_t *stats8);

/* Page-locked host memory for buffers that cross PCIe (reads in, ranked hits or CSR out).  NULL when it cannot be had. */
void *kasa_host_alloc(size_t bytes);
void kasa_host_free(void *p);
/* Plain device memory for a host that keeps its inputs resident in HBM (kasa_batch_upload_device) and holds no other GPU
 * library: allocate, fill from host memory, free.  Ours (the reference has no device): bench.py's one-GPU run keeps its reads
 * in these, so that process never imports torch and the library runs on the HIP runtime it was built for. */
int kasa_device_alloc(int device, size_t bytes, void **out);
int kasa_device_free(int device, void *p);
int kasa_device_write(int device, void *dst, const void *src, size_t bytes);
int kasa_device_read(int device, void *dst, const void *src, size_t bytes);
/* Device memory to device memory, on one device or between two; no peer access is needed (or enabled).  Returns when the bytes
 * are there.  Not a context call: host threads may copy into disjoint places of one buffer at the same time (the partitions'
 * records into the owner's kasa_batch_records_inbox). */
int kasa_device_copy(int dstDevice, void *dst, int srcDevice, const void *src, size_t bytes);
/* Binds the CALLING host thread to a device.  A fresh thread stands on device 0, and kasa_host_alloc page-locks for the
 * thread's current device: a helper thread that prepares a worker's buffers calls this first (the kasa_ctx_* / kasa_batch_*
 * calls select their context's device themselves). */
int kasa_thread_device(int device);

/* ---- profile tables: vCount_all / vCount_unique / vCount_total (Compare.hpp:2830-2839) ---------- */
int kasa_profile_reset(kasa_ctx *ctx);
/* dst += src, src = 0.  The profile of a batch is made where its queries are GROUPED (kasa_batch_lookup_score, kasa_batch_group):
 * a sum over (group, taxon) of the group's hits (Compare.hpp:922-925), from the sorted queries -- with 32-byte records (up to 8
 * levels) kasa_batch_score adds nothing to the tables; with 64-byte records (9-25 levels, the 128-bit index's default k range)
 * the profile still comes from the per-read side, i.e. from kasa_batch_score.  A context that groups slices for another one
 * (the partition worker of a range-partitioned index) hands its tables on with this call.  Same k range and taxa; the two
 * contexts may sit on different devices (src's tables are copied to dst's device and added there -- one path for both cases,
 * exact integer sums).  This is also how the owners of a file's batches are summed in one process without a communicator. */
int kasa_profile_absorb(kasa_ctx *dst, kasa_ctx *src);
/* countAll as double (exact 64.64 fixed-point sums rounded once), countUnique, countTotal; any may
 * be NULL.  nK * nTaxa entries each. */
int kasa_profile_fetch(kasa_ctx *ctx, double *countAll, uint64_t *countUnique, uint64_t *countTotal);
/* The same tables as 6 integer limbs per cell {unique, total, all[0..3] (32 bits each, little
 * endian)} so that ranks can be summed with a plain integer reduce (the thread reduce of
 * Compare.hpp:3445-3454 across GPUs); import REPLACES the context's tables by the limbs handed in
 * (the sum over all ranks, after the reduce). */
int kasa_profile_export_limbs(kasa_ctx *ctx, uint64_t *limbs);
int kasa_profile_import_limbs(kasa_ctx *ctx, const uint64_t *limbs);
/* The whole reduce on the device: limbs packed in HBM, ONE ncclAllReduce (u64, sum; exact and order-independent) on
 * the context's stream over the communicator handed in (an ncclComm_t of RCCL, passed as void * so that this header
 * needs no RCCL include), carries folded back.  Afterwards every rank's tables hold the global sums.  Collective:
 * every rank of the communicator must call it. */
int kasa_profile_allreduce(kasa_ctx *ctx, void *rcclComm);
/* RCCL is bound at run time to the copy the process already holds -- the one that made `rcclComm` (the host's own link,
 * a torch wheel's bundled librccl, a ctypes load); librccl.so.1 is loaded only when the process has none.  What this
 * library was built with and what it runs on: HIP versions as HIP_VERSION (major * 10^7 + minor * 10^5 + patch), RCCL's as
 * NCCL_VERSION_CODE; *rcclRuntime = 0 when no RCCL is in the process.  Any pointer may be NULL.  (No reference
 * counterpart: kASA is one statically linked binary; this is what lets a host that shares its process with another ROCm
 * stack see a mismatch instead of running on it unawares.) */
int kasa_runtime_versions(int *hipBuilt, int *hipRuntime, int *hipDriver, int *rcclBuilt, int *rcclRuntime);

/* ---- measurement + test taps ------------------------------------------------------------------ */
/* HIP-event time (ms) and launch count of a stage, accumulated since the last reset. */
int kasa_ctx_stage_ms(kasa_ctx *ctx, int stage, double *ms, uint64_t *launches);
int kasa_ctx_stage_reset(kasa_ctx *ctx);
/* HIP-event time of single kernels alone (accumulated since the last kasa_ctx_stage_reset), for the roofline lines. */
enum {
    KASA_KERNEL_LOOKUP = 0,       /* lookup_tile_kernel: the sorted-index lookup */
    KASA_KERNEL_GROUP = 1,        /* group_kernel: flush order + taxon segments, one record per query */
    KASA_KERNEL_SCORE_MAIN = 2,   /* score_main_kernel: the float chains of a read's register taxa */
    KASA_KERNEL_SCORE_OTHER = 3,  /* score_other_flat_kernel / score_other_flat16_kernel (debug bit 5: score_other_kernel): staging records of all other taxa */
    KASA_KERNEL_ROW_MERGE = 4,    /* row_merge_*: staging rows -> final {taxon, score} rows + profile keys */
    KASA_KERNEL_SCORE_GENERAL = 5,/* flush_positions_kernel + score_kernel (all its passes): the reads the fast kernels hand over */
    KASA_KERNEL_PROFILE_TABLES = 6,/* profile_(group_)table_kernel + the sort and reduce of the keys it leaves over */
    KASA_KERNEL_ROW_COPY = 7,     /* row lengths -> CSR offsets (scan) + row_copy_kernel */
    KASA_KERNEL_SORT_PASSES = 8,  /* kasa_radix: hist_kernel + the radix passes of the query sort */
    KASA_KERNEL_BUCKET_RANK = 9,  /* bucket_rank*_kernel: the query sort's last step */
    KASA_KERNEL_SCORE_DENSE = 10, /* score_dense_kernel: reads with long rows that keep the fast kernels' order rule (crowded indices) */
    KASA_KERNEL_SCORE_REPLAY = 11,/* kasa_replay.h: very long reads -- events sorted by (read, taxon, flush position, level), float chains per (read, taxon) */
    KASA_KERNEL_COUNT = 12
};
int kasa_ctx_kernel_ms(kasa_ctx *ctx, int kernel, double *ms, uint64_t *launches);
/* Of the last batch: {queries, staging records, profile keys, pool words, reads on the general kernel, of those on its
 * second pass, non-zero score cells, 1 if the encoder ranked the reads' k-mers (no slot fix-up)}. */
int kasa_ctx_batch_stats(kasa_ctx *ctx, uint64_t *stats8);
/* Of the last batch's group stage: the tiles of 1024 sorted queries it had, and how many of them the dense-leader kernel
 * (group2_kernel) left to the general one -- tiles with long taxon lists (Compare.hpp:396-441, a conserved k-mer) or walks
 * beyond its staged index span; 0 when the general kernel ran alone. */
int kasa_ctx_group_tiles(kasa_ctx *ctx, uint32_t *tiles, uint32_t *listed);
/* Of the last batch's score stage: the reads score_dense_kernel scored -- reads with long rows (many taxa per k-mer:
 * Compare.hpp:396-441) whose groups all close before the read's next matched query, replayed query by query from the row in
 * LDS; the others of the fast kernels' leftovers are the general kernel's (kasa_ctx_counters). */
int kasa_ctx_dense_reads(kasa_ctx *ctx, uint32_t *denseReads);
/* Number of query records the batch holds right now: the k-mer count of kasa_batch_encode, less the
 * duplicates once kasa_batch_sort_and_range ran with unique != 0. */
int kasa_batch_query_count(kasa_ctx *ctx, uint64_t *n);

/* Queries of the batch after encode / after sort (k-mer, read id); for parity tests.  A k-mer is one
 * uint64_t with a 64-bit index, two (low word, high word) with a 128-bit index. */
int kasa_batch_fetch_queries(kasa_ctx *ctx, void *kmers, uint32_t *reads, uint64_t n);
/* Test tap: the payload word of every query as kasa_batch_encode left it, in emission order -- the query's slot in the
 * read-major, sorted-within-read record array where the encoder ranked the reads' k-mers (kasa_ctx_batch_stats: stats8[7]
 * = 1), the read id otherwise.  A plain copy to the host: no kernel runs, nothing of the batch changes.  KASA_E_STATE unless
 * the batch was encoded by kasa_batch_encode and not sorted yet (the sort moves and then replaces these words). */
int kasa_batch_fetch_payload(kasa_ctx *ctx, uint32_t *out, uint64_t n);
/* Test tap: install (k-mer, read id) queries directly instead of upload + encode (any order). */
int kasa_batch_set_queries(kasa_ctx *ctx, const void *kmers, const uint32_t *reads, uint64_t n, int64_t nReads);
/* Test tap (like kasa_batch_set_queries and kasa_text_dtoa): replace the per-read score rows of the batch that is loaded
 * by a CSR of the caller's -- readOffsets[nReads + 1], per read taxIdx strictly ascending (the rank kernels index the
 * denominators with them) and any float as score, zeros, infinities and NaN included.  kasa_batch_scores_fetch then returns
 * exactly these arrays, kasa_batch_rank and kasa_batch_text work on them; rank and text results of the batch become invalid,
 * its coherence scores stay.  Works on any loaded batch, whatever has run on it (right after kasa_batch_upload, too).
 * KASA_E_STATE: no batch is loaded.  KASA_E_ARG: nReads is not the batch's read count; the offsets do not start at 0 or
 * descend; a taxon index >= the index's taxon count; taxon indices not strictly ascending within a row. */
int kasa_batch_set_scores(kasa_ctx *ctx, const uint64_t *readOffsets, const uint32_t *taxIdx, const float *score, uint64_t nReads);
/* Per sorted query: deepest matched level k (0 = none) and an index position sharing that prefix. */
int kasa_batch_fetch_lookup(kasa_ctx *ctx, uint8_t *depth, uint32_t *indexPos, uint64_t n);
int kasa_ctx_device_bytes(kasa_ctx *ctx, uint64_t *bytes);
/* Sizing a batch (the reference sizes its batches by -m, Compare.hpp:2803-2876): free / total HBM of a device, and the
 * device bytes one query k-mer costs while its batch is in flight (all stages resident). */
int kasa_device_memory(int device, uint64_t *freeBytes, uint64_t *totalBytes);
uint64_t kasa_batch_bytes_per_query(const kasa_ctx *ctx);

/* ---- where the reference cuts its batches (host arithmetic, no device work) ---------------------------------------
 * Per-read scores are float sums whose order depends on the reads that share a batch, so byte-identical per-read files
 * need the reference's batch boundaries: `kASA identify -m <GB>` turns -m into a byte budget
 * (main.cpp:438-447,590-592,1054-1060; Compare.hpp:111-160,182-328,2803-2818,3129-3132) that every read consumes
 * (Read.hpp:612-630,1147,1165-1195).  A host calls kasa_refbatch_budget once, kasa_refbatch_sequence_cost / _read_overhead per read and
 * kasa_refbatch_cut per batch; the device takes whatever batch it is handed. */
typedef struct {
    int64_t memoryGiB;            /* -m (0: the default, 5) */
    int threads;                  /* -n */
    int ram;                      /* -r */
    int kHigh, kLow;
    int recordBytes;              /* of the index FILE: 12, 20 (128-bit) or 6 (halved) */
    uint64_t nRecords;
    const uint32_t *triePrefix;   /* the `_trie` file's prefixes, ascending */
    uint64_t nTrie;
    const uint32_t *taxIds;       /* as for kasa_index_create: entry 0 = 0 */
    uint32_t nTaxa;
    uint64_t nameBytes;           /* bytes of all names of the content file after removing ',' (entry 0 not counted) */
    int identifyMultiple;         /* main.cpp:1118-1334 */
} kasa_refbatch_params;
int kasa_refbatch_budget(const kasa_refbatch_params *p, int64_t *budget);
/* One sequence (a read, or one mate of a pair): K = 12 or 25 (index type), mode 0 = DNA in 3/6 frames, 1 = --one,
 * 2 = amino acids; strands = 2 with --six.  The read as a whole, when per-read results are kept (-q / --filter):
 * nameLen = length of the specifier the reference stores (header without its first character + one space; both mates').
 * coherence: --coherence widens the k-mer records (InputType::ppTuple, MetaHeader.h:172) and adds a float per read
 * (Read.hpp:1191-1193). */
int64_t kasa_refbatch_sequence_cost(int K, int kLow, int mode, int strands, int64_t rawLen, int coherence);
int64_t kasa_refbatch_read_overhead(int64_t nameLen, uint32_t nTaxa, int coherence);
/* Reads of the next batch given the costs of the reads still to come. */
uint64_t kasa_refbatch_cut(int64_t budget, int firstBatch, const int64_t *cost, uint64_t nReads);

/* Device buffers for a batch of about nQueries k-mers out of nBases bases, before the batch is there: allocation takes
 * 25-90 ms per GB on this platform (seconds for a 10 M-read batch), time a host has while it parses its input.  Sizes only --
 * a batch that needs more gets more when it arrives.  Not while a batch of this context is in flight. */
int kasa_ctx_reserve(kasa_ctx *ctx, uint64_t nQueries, uint64_t nBases, int wantPerRead);

/* Of the last batch: reads scored by the general kernel (score_kernel) instead of the lane-per-read one, and how many of
 * those needed its second pass (full pending window / direct profile adds).  Diagnostics for tests and bench.py. */
int kasa_ctx_counters(kasa_ctx *ctx, uint32_t *generalReads, uint32_t *secondPassReads);
/* ... and how many of those kept more groups pending than the second pass's window holds (4096) and were ordered through a
 * window in device memory (narrow records; 64-byte records return KASA_E_LIMIT there).  Ours: the reference's flush is a
 * hash map per thread and has no such window (Compare.hpp:917-955). */
int kasa_ctx_third_pass_reads(kasa_ctx *ctx, uint32_t *thirdPassReads);
/* Of the last batch's score stage (its last attempt, where the staging buffer grew): why score_main_kernel handed reads to
 * the slower kernels.  out[0]: more k-mers than the counters' fields hold (255, or 60 000 with 16-bit fields); [1]: too many
 * taxa (no kernel of this build counts it: always 0); [2]: a staging row longer than the row merge takes; [3]: a list of 8192 or more segments; [4]: the order rule (an
 * earlier group of the read is still open at its next matched query).  Read-only: a copy of counters the kernel keeps anyway.
 * Diagnostics for tests. */
int kasa_ctx_hand_over_reasons(kasa_ctx *ctx, uint32_t out[5]);
/* The row merge takes the staging rows of the fast score kernels in classes by length (256 / 512 / 1024 records up to 2048
 * taxa, 256 / 1024 up to 16 384 taxa where the second class stays empty, and a streaming class for the longer rows of long
 * reads): the first class's launch sweeps all reads, the others walk the rows score_main_kernel listed for them and are not
 * launched without any.  out[0..3]: rows of the last batch in the first, second, third and long class (the first counts
 * every read the fast kernels kept that is not listed above it, rows without records included; zeros when the sorting merge
 * or the general kernel took the batch -- the first then holds the reads the fast kernels kept).  Diagnostics, host side only. */
int kasa_ctx_row_classes(kasa_ctx *ctx, uint64_t out[4]);
/* Test tap: at most n workgroups per row-merge launch (0: as many as are resident), so that a small batch makes one
 * wavefront walk many rows. */
int kasa_ctx_row_merge_blocks(kasa_ctx *ctx, uint32_t n);
/* Test tap: on != 0 makes every later kasa_batch_score / kasa_batch_lookup_score copy the rows' lengths to the host before
 * the merge replaces them by the number of distinct taxa (one more copy and wait per batch); kasa_batch_staged_lengths
 * returns them, out[nReads]: records of a row the fast kernels staged, pairs of a row the general kernel wrote. */
int kasa_ctx_keep_staged_lengths(kasa_ctx *ctx, int on);
int kasa_batch_staged_lengths(kasa_ctx *ctx, uint32_t *out);
/* ... and the reads of that list that were long enough (16384 k-mers and more: a contig, a chromosome read in pieces under one
 * read id) to be replayed from SORTED EVENTS instead -- every query of theirs turned into events {read, taxon, flush position,
 * level} by all wavefronts, one radix sort, one float32 chain per (read, taxon) -- and the events that took.  The reference
 * streams such a sequence at merge speed (Compare.hpp:747-1043; pieces: Read.hpp:437-443,678-695); one wavefront per read
 * does not.  Both record widths (64-byte records: the replay also adds the events to the profile tables). */
int kasa_ctx_replay_stats(kasa_ctx *ctx, uint32_t *reads, uint64_t *events);
/* Of the tiles kasa_ctx_group_tiles reports as listed by the dense-leader kernel: those that its second launch -- the same
 * kernel with a park buffer four times as large, for tiles that only parked too many segments (a heavy 7-letter group) --
 * listed AGAIN and left to the cooperative kernel (long taxon lists, walks beyond the staged index span).  Ours. */
int kasa_ctx_group_second_chance(kasa_ctx *ctx, uint32_t *listedAgain);
/* How the buffer of 32-byte event records was chosen.  The rate at which an MI355X takes random 32-byte stores is a property
 * of the physical memory behind a buffer (21 to 28 G records/s, tools/place_probe.hip), and the group stage ends in one such
 * store per query: a buffer of 8 GB and more (KASA_PLACE_MIN_MB) is taken from up to three candidates (KASA_PLACE_TRIES),
 * each timed with a few milliseconds of scattered stores when it is allocated.  candidates = 0: allocated plainly (a small
 * buffer, 64-byte records); keptRate and rates4[0..3] in G records/s.  rates4 may be NULL.  Ours: the reference has no
 * device memory (its record of a k-mer's hits is the host vector of Compare.hpp:1430-1467). */
int kasa_ctx_record_placement(kasa_ctx *ctx, uint32_t *candidates, float *keptRate, float *rates4);

/* Test tap: forceSlowScore >= 0 is a bit set: bit 0 = every read takes the general (wavefront-per-read)
 * score kernel, bit 1 = per-query index search instead of the streamed-tile lookup, bit 2 = sorting row
 * merge instead of the bitmap one, bit 3 = the encoder does not rank the k-mers of a read (slots come from
 * a stable sort by read id, as for long or paired reads), bit 4 = the profile keys are sorted and reduced even
 * when the LDS counting table would fit, bit 5 = score_other_kernel (one lane per query, either record width) instead of
 * score_other_flat_kernel / score_other_flat16_kernel (work items = segments), bit 6 = the library's radix sort over all
 * key bits instead of 4 (5) passes + bucket_rank_kernel, bit 7 = long sort buckets are not sorted one by one but by the
 * library over all bits (the path for inputs with too many or too long ones), bit 8 = kasa_batch_rank leaves reads with
 * tied hits to the host instead of ranking them with std::sort's order on the device, bit 9 = the library's radix passes
 * over the top 32 (40) key bits instead of the hand-written ones (kasa_amd/csrc/kasa_radix.h), bit 10 = score_main_kernel with the
 * next line of records prefetched into registers (fewer resident wavefronts), bit 11 = no followers (every query walks the
 * index itself), bit 12 = 64-byte records without the index span in LDS, bit 13 = the general score kernel in its
 * lane-owns-its-cells form (what indices beyond 16 384 taxa take) instead of the row in LDS, bit 14 = the general kernel's
 * first pass hands every read to its second pass, bits 15 / 16 = timing taps of group_kernel (no profile keys at all; keys
 * counted but not stored: the profile is wrong), bit 17 = never the cooperative form of group_kernel (long taxon lists lane
 * by lane; level sizes beyond 255 wrap), bit 18 = the cooperative form from the first batch on, bit 19 = the radix passes of the
 * query sort look back over the earlier tiles before they order their keys in LDS (the form of rounds 2-3), bit 20 =
 * rank_exact_kernel in its largest form for every read (no classes by hit count), bit 21 = the other split of the query
 * sort (64-bit keys: five passes over 40 bits + buckets of 20 bits' worth; 128-bit keys: four passes over 32 bits + buckets
 * of 93), bit 22 = the bucket pass of 64-bit keys by the kernel for any key width, bit 23 = the general kernel's second pass
 * hands every read to its third (pending window in device memory; narrow records), bit 27 = narrow records are stored as
 * whole 64-byte cells (group2_kernel writes the record and 32 bytes of zeros by lane quads: a layout option, also
 * KASA_WIDE_CELLS=1), bit 29 = never the sorted-event replay of very long reads (kasa_ctx_replay_stats), bit 30 = that replay for
 * every read of the general kernel's list, whatever its length; lastSlowReads (may be
 * NULL) receives how many reads of the last batch took the general score kernel. */
int kasa_ctx_debug(kasa_ctx *ctx, int forceSlowScore, uint32_t *lastSlowReads);
int kasa_ctx_synchronize(kasa_ctx *ctx);

/* ---- build: the index files from a database, on the device -----------------------------------------------------------
 * kASA's `build` (main.cpp:628-686 -> kASA.hpp:449-575 BuildAll): sequences tagged with tax IDs -> every '^'-padded window
 * of K letters (Read.hpp:2928-3176), sorted by (k-mer, tax ID) and made unique (Build.hpp:305-477), the prefix trie of 6
 * letters (Trie.hpp:365-394) and the frequency rows of `_f.txt` (kASA.hpp:517-526).  The reference goes through in-RAM
 * bricks, STXXL temporary files and a k-way merge; here a brick is encoded, sorted and made unique on the device, its run
 * stays in device memory, and the runs are merged there.
 *   kasa_build_create  K = 12 (64-bit index) or 25 (128-bit, --kH 25); frames = 3, or 1 (--one); codonLut = NULL: the built-in
 *                      table (-a gc.prt id: the host's table over kasa_builtin_codon_table); taxIds[nTaxa] = the content file's tax IDs
 *                      (entry 0 = 0, as for kasa_index_create; nTaxa < 2^22); maxPairsPerBrick = pairs the encoder emits
 *                      per brick (0 = automatic, from the device's free memory; tests force many bricks on tiny inputs).
 *   kasa_build_add     any number of calls, as a parser hands sequences over: nSeq sequences (bases, offsets[nSeq + 1]),
 *                      seqTaxId[s] one of taxIds (KASA_E_ARG otherwise: unknown accessions are the host's to skip,
 *                      Read.hpp:2352-2368), protein = amino-acid letters (kASA::detectAlphabet per file).
 *   kasa_build_finish  the last brick, the merges (a result that does not fit the device with one merge buffer is built by
 *                      slabs, see "indices larger than device memory" below; KASA_E_LIMIT only for a builder with edits, or
 *                      when a single 6-letter prefix exceeds a slab), records, trie and frequencies.  nRecords = unique (k-mer, tax ID) entries, nTrie =
 *                      trie entries.
 *   kasa_build_fetch   records: nRecords packed file records, 12 bytes {u64 kmer, u32 taxid} or 20 bytes {u64 lo, u64 hi,
 *                      u32 taxid}; triePrefix / trieCount: nTrie entries of the `_trie` file; freq: nTaxa x K, row r =
 *                      content row r, column j = entries whose letter j from the right is not '^' (k = K - j).  Any may
 *                      be NULL.  kasa_build_fetch_range: records [first, first + count) only (a host writes while it copies).
 *   kasa_build_stats   stats8 = {pairs in, bricks, merges of two runs, records out, device microseconds of encode,
 *                      sort + unique, merge, emit (records, trie, frequencies)}.
 * Counts and offsets are 64-bit: the 2^32-record limit of kasa_index_create is identify's, not the build's. */
typedef struct kasa_builder kasa_builder;
int kasa_build_create(int device, int K, int frames, const uint8_t *codonLut, const uint32_t *taxIds, uint32_t nTaxa,
                      uint64_t maxPairsPerBrick, kasa_builder **out);
int kasa_build_add(kasa_builder *b, const uint8_t *bases, const int64_t *offsets, int64_t nSeq, const uint32_t *seqTaxId, int protein);
int kasa_build_finish(kasa_builder *b, uint64_t *nRecords, uint64_t *nTrie);
int kasa_build_fetch(kasa_builder *b, void *records, uint32_t *triePrefix, uint64_t *trieCount, uint64_t *freq);
int kasa_build_fetch_range(kasa_builder *b, uint64_t first, uint64_t count, void *records);
int kasa_build_stats(kasa_builder *b, uint64_t *stats8);
void kasa_build_destroy(kasa_builder *b);

/* ---- edit: update, delete, shrink and merge existing indices, on the device-----------------------------------------------
 * kASA's `update` (Update.hpp:99-180: the sorted union of the old records and those `build` makes of new sequences),
 * `delete` (Update.hpp:28-90: the records of the taxa delnodes.dmp does not list, in order), `shrink` (Shrink.hpp:152-370)
 * and `getFrequency` (main.cpp:1336-1362) on a builder.  An existing index is one more sorted run: kasa_build_finish merges
 * the brick runs, then every index run once with that result, then drops the taxa, then shrinks, then writes records,
 * trie and frequencies as for a build.  A builder that calls none of these behaves as before.
 *   kasa_build_add_index   records [first, first + count) of an index run of `total` packed file records (12 or 20 bytes,
 *                          as kasa_build_fetch writes them, the width of the builder's K).  first = 0 starts a run; the calls
 *                          of a run cover [0, total) in order.  KASA_E_ARG names the record and its tax ID when the tax ID
 *                          is not one of taxIds, or when a record does not follow its predecessor in strict (k-mer, tax
 *                          ID) order (unsorted input, a duplicate); the run is then discarded.
 *   kasa_build_drop_taxa   the records of these tax IDs go (delete -l delnodes.dmp).  Calls combine as a union; IDs that no
 *                          record carries are ignored.
 *   kasa_build_shrink      once per builder.  strategy 1: per taxon, the j-th record in index order (j = 1, 2, ...) goes iff
 *                          j == (uint64_t)d_m for some m, d_1 = step = 100.0 / fabsf(percentage) in double, d_m+1 = d_m +
 *                          step (no record goes when step < 1 or percentage = 0).  2: the halved index (64-bit K only, at most
 *                          65535 content rows with row 0): records whose six low letters are all '^' go, the others are
 *                          fetched as 6-byte records {u32 low 30 bits of the k-mer, u16 content row} and the frequencies
 *                          are those of the full index.  3: records whose normalised Shannon entropy of the K letters
 *                          ('^' included) is 0.5 or less go.  A shrink that leaves no record fails kasa_build_finish
 *                          with KASA_E_ARG.
 *   kasa_build_edit_stats  stats4 = {index records in, dropped by delete, dropped by shrink, device microseconds of the
 *                          loads and the filters}.  With several index runs {0} counts the records of all of them.
 *   kasa_build_taxa_histogram  `redundancy` (Shrink.hpp:35-72), valid after kasa_build_finish, on the final sorted records:
 *                          hist[c], 1 <= c < nBins, = the distinct k-mers that carry exactly c records (c tax IDs); hist[0] = 0;
 *                          *distinctKmers = the sum of the bins.  KASA_E_STATE before the finish and on a halved result
 *                          (shrink strategy 2: its records keep 30 bits of a k-mer).  KASA_E_ARG when a k-mer carries more
 *                          than nBins - 1 records, which nBins = nTaxa + 1 rules out: (k-mer, tax ID) pairs are unique.
 * `merge` is two kasa_build_add_index runs (first = 0 starts the second once the first is complete) and no filter: the finish
 * merges them and drops the records both hold.  `trie` is one index run whose caller fetches only triePrefix and trieCount
 * (kasa_build_fetch with records = NULL, freq = NULL copies no record down). */
int kasa_build_add_index(kasa_builder *b, uint64_t first, uint64_t count, uint64_t total, const void *records);
int kasa_build_drop_taxa(kasa_builder *b, const uint32_t *taxIds, uint64_t n);
int kasa_build_shrink(kasa_builder *b, int strategy, float percentage);
int kasa_build_edit_stats(kasa_builder *b, uint64_t *stats4);
int kasa_build_taxa_histogram(kasa_builder *b, uint64_t *hist, uint64_t nBins, uint64_t *distinctKmers);

/* ---- build: indices larger than device memory ---------------------------------------------------------------------------
 * The reference builds any size through STXXL temporaries (Build.hpp:305-477).  Here the bricks' runs leave the device for
 * ordinary (pageable) host memory once they outgrow a resident budget, and the finish walks the key space in slabs: intervals
 * of 6-letter trie prefixes, so that no k-mer, duplicate pair or trie entry is split.  A slab's slices are uploaded, merged,
 * emitted and trie'd; the frequency histograms live across the slabs.  The slabs' records and trie entries concatenate to the
 * index.  There is one finish: a builder whose runs stayed on the device has one slab, all of its records, made by the same code.
 *   kasa_build_set_resident  before the first kasa_build_add (KASA_E_STATE after it, and after an edit call):
 *                          maxResidentRecords = the most input records a slab may bring to the device.  0 (the default) =
 *                          automatic: the builder spills once the in-core finish of the runs it holds is no longer sure to
 *                          fit (36 bytes per record with 64-bit keys, 52 with 128-bit, against 0.8 of the free memory), or
 *                          when the finish's memory check refuses a merge, and sizes the slabs by the same arithmetic.
 *                          Otherwise: as soon as the runs on the device hold more records than this they go to the host,
 *                          and every later run follows.
 *   kasa_build_finish_begin  the last brick; then, runs on the device: the merges, the edits and the one slab; runs in host
 *                          memory: the plan.  *nSlabs = the slabs to take.  KASA_E_LIMIT names the prefix, its input records
 *                          and the budget when one prefix alone exceeds the budget; KASA_E_NOMEM when the host has no
 *                          memory for a run.
 *   kasa_build_slab        slab 0, 1, .. nSlabs - 1 in order, each once (KASA_E_STATE otherwise): *nRecords and *nTrie of
 *                          this slab.
 *   kasa_build_fetch_slab  records [first, first + count) of the current slab and its trie entries (all nTrie of them);
 *                          any pointer may be NULL.
 *   kasa_build_finish_end  after the last slab: the totals.  Then kasa_build_fetch(b, NULL, NULL, NULL, freq) gives the
 *                          frequency rows.
 *   kasa_build_spill_stats stats8 = {runs spilled, records spilled, slabs, the largest slab's input records, the heaviest
 *                          prefix's input records, host microseconds of the copies host -> device, device -> host, 0}; all
 *                          zero for a builder that did not spill.
 * kasa_build_finish is kasa_build_finish_begin, every kasa_build_slab and kasa_build_finish_end in one call.  On a builder that
 * did not spill, kasa_build_finish_begin does all the work of kasa_build_finish and reports one slab, kasa_build_slab(b, 0)
 * returns the totals and kasa_build_fetch_slab is kasa_build_fetch_range plus the trie: a host needs one code path, and edited
 * builders (update, delete, shrink, merge) take it too.
 * kasa_build_finish on a builder that spilled gathers the records and trie of every slab in host memory, so
 * kasa_build_fetch and kasa_build_fetch_range keep working, bounded by the host's RAM; after the streaming calls they return
 * KASA_E_STATE for records and trie.  kasa_build_stats' merges counts the merges of all slabs.
 * Edits need the runs on the device: kasa_build_add_index, kasa_build_drop_taxa and kasa_build_shrink return KASA_E_STATE on a
 * builder with a non-zero budget or spilled runs, a builder with edits never spills (KASA_E_LIMIT as before), and
 * kasa_build_taxa_histogram returns KASA_E_STATE after a spilled finish. */
int kasa_build_set_resident(kasa_builder *b, uint64_t maxResidentRecords);
int kasa_build_finish_begin(kasa_builder *b, uint64_t *nSlabs);
int kasa_build_slab(kasa_builder *b, uint64_t slab, uint64_t *nRecords, uint64_t *nTrie);
int kasa_build_fetch_slab(kasa_builder *b, uint64_t first, uint64_t count, void *records, uint32_t *triePrefix, uint64_t *trieCount);
int kasa_build_finish_end(kasa_builder *b, uint64_t *nRecords, uint64_t *nTrie);
int kasa_build_spill_stats(kasa_builder *b, uint64_t *stats8);

/* ---- parse: FASTA / FASTQ text -> reads, on the device ------------------------------------------------------------------
 * The producer of what kasa_batch_upload_device takes: the text of whole records goes in, the reads come out in device
 * memory -- what Read::readFastqa / readFasta (Read.hpp:699-760) hand on for reads that fit one chunk, byte for byte what the
 * host driver's parseRecords makes of the same text:
 *   bases    the sequence lines back to back without their line feeds, untouched (a '\r' stays part of its line; cleaning and
 *            case folding are the encoder's, Read.hpp:633-675)
 *   off      [nReads + 1] running offsets into bases
 *   names    header without its first character plus one space (Read.hpp:711-714), back to back, with nameOff[nReads + 1]
 *   lengths  letters plus one per sequence line (Read.hpp:723-731); FASTA counts the non-empty sequence lines
 * A kasa_parser is a POOL of parsed reads on one device, single-threaded like a context.
 *   kasa_parse_create   longSequence: records of that many letters and more are not taken (the reference reads them in
 *                       pieces, Read.hpp:371-600; the host driver's KASA_LONG_SEQUENCE, 1000000 by default).
 *   kasa_parse_append   text: host memory (page-locked memory crosses PCIe fastest), nBytes of WHOLE records: it starts at a
 *                       header line and only its last line may lack a line feed.  fasta: '>' records, else '@' records of
 *                       strictly four lines.  The reads go behind those pooled so far: consecutive chunks of a file form one
 *                       running read set.  *parsable = 0: the chunk is not in the form the device takes -- the pool is left
 *                       exactly as it was, *nReadsAdded = 0, the call returns KASA_OK, and the caller parses the chunk itself
 *                       (so every message about malformed input keeps coming from the host parser).  kasa_parse_status names
 *                       the first offending property (KASA_PARSE_*) and its chunk position: the start of the line that has it
 *                       (KASA_PARSE_LONG: of the record's header), for KASA_PARSE_BLANK the space or tab itself.
 *   kasa_parse_sizes    reads, letters and name bytes pooled right now.
 *   kasa_parse_fetch    reads [first, first + n) of the pool to host memory; any pointer may be NULL; off and nameOff are
 *                       rebased to `first` (off[0] = nameOff[0] = 0).  One 32-byte read-back for the range's ends, then the copies.
 *   kasa_parse_take     the first nReads pooled reads become ctx's batch and leave the pool: the context gets its own
 *                       device-to-device copy of the bases (the pool's memory is reused by the next append, while a batch's
 *                       bases must stay valid until its last call) and goes on as kasa_batch_upload_device does (geometry on the
 *                       device, one 8-byte read-back), after one 32-byte read-back of its own for where the reads left behind
 *                       start.  KASA_E_ARG when the context is on another device than the pool.
 *   kasa_parse_tile_bytes  bytes of text (and of output) one wavefront owns: tests size their inputs by it.
 *   kasa_parse_stage_ms  HIP-event milliseconds, summed over the appends: text upload, and the kernels from line table to gather. */
enum {
    KASA_PARSE_OK = 0,
    KASA_PARSE_FASTQ_LINES = 1,     /* the line count of a FASTQ chunk is not a multiple of 4 */
    KASA_PARSE_FASTQ_HEADER = 2,    /* line 0 of a FASTQ record does not start with '@' */
    KASA_PARSE_FASTQ_PLUS = 3,      /* line 2 of a FASTQ record does not start with '+' */
    KASA_PARSE_FASTQ_QUALITY = 4,   /* the quality line differs in length from the sequence line */
    KASA_PARSE_EMPTY_LINE = 5,      /* an empty line in a FASTQ chunk */
    KASA_PARSE_BLANK = 6,           /* a space or tab in a sequence line */
    KASA_PARSE_LONG = 7,            /* a record of longSequence letters or more */
    KASA_PARSE_FASTA_HEADER = 8,    /* a FASTA chunk that does not start with '>' */
    KASA_PARSE_FASTQ_SEQ_PLUS = 9,  /* a FASTQ sequence line that starts with '+' (the host parser takes it for the '+' line) */
    KASA_PARSE_TOO_LARGE = 10,      /* a chunk of 4 GiB or more (positions in a chunk are 32-bit) */
    KASA_PARSE_INFLATE = 11         /* kasa_bgzf_parse_append: a member does not inflate; `at` is the member's index in the span */
};
typedef struct kasa_parser kasa_parser;
int kasa_parse_create(int device, uint64_t longSequence, kasa_parser **out);
int kasa_parse_append(kasa_parser *p, const char *text, uint64_t nBytes, int fasta, uint64_t *nReadsAdded, int *parsable);
int kasa_parse_status(kasa_parser *p, int *code, uint64_t *at);
const char *kasa_parse_status_text(int code);
int kasa_parse_sizes(kasa_parser *p, uint64_t *nReads, uint64_t *nBases, uint64_t *nNameBytes);
int kasa_parse_fetch(kasa_parser *p, uint64_t first, uint64_t n, uint32_t *lengths, uint64_t *nameOff, char *names, int64_t *off, uint8_t *bases);
int kasa_parse_take(kasa_parser *p, kasa_ctx *ctx, uint64_t nReads);
int kasa_parse_tile_bytes(void);
int kasa_parse_stage_ms(kasa_parser *p, double *uploadMs, double *parseMs);
/* The same pool fed with BGZF (kasa_bgzf_inflate above): a span of WHOLE members goes up compressed, is inflated into the
 * parser's text buffer behind what the previous call carried, and the text is cut ON THE DEVICE at its last whole record --
 * FASTQ: behind the last line feed that closes a fourth line (lines counted from the text's start: the carry begins a record),
 * FASTA: before the last line that begins with '>' (its record may go on in the next span); final != 0: nothing is cut.  The
 * cut text is parsed as kasa_parse_append parses a chunk, from the same line table and without a second upload; what lies
 * behind the cut is carried: it moves to the front of the text buffer for the next call.
 *   *nReadsAdded  reads pooled by this call; 0 with *parsable = 1 when the text holds no whole record yet (a contig that spans
 *                 many members): everything is carried
 *   *nTextBytes   bytes of text this call parsed (over a file they sum to its inflated size), *carryBytes what is carried now
 *   *parsable = 0 the pool AND the carry are as before the call.  KASA_PARSE_INFLATE: a member of the span is malformed --
 *                 kasa_bgzf_parse_status gives its KASA_INFLATE_* code and its index in the span (kasa_parse_status' `at`
 *                 too); KASA_PARSE_TOO_LARGE: carry plus span reach 4 GiB; every other code as for kasa_parse_append, `at`
 *                 counted in the cut text (carry included).
 * kasa_parse_append returns KASA_E_STATE while bytes are carried.  kasa_bgzf_parse_ms: HIP-event milliseconds of the inflate
 * kernels, summed like kasa_parse_stage_ms' two (the upload there is then the compressed bytes'). */
int kasa_bgzf_parse_append(kasa_parser *p, const void *members, uint64_t nBytes, int fasta, int final, uint64_t *nReadsAdded, int *parsable,
                           uint64_t *nTextBytes, uint64_t *carryBytes);
int kasa_bgzf_parse_status(kasa_parser *p, int *code, uint64_t *member);
/* The same pool fed with a PLAIN gzip file (kasa_gzip_inflate above): spans of the file's bytes as they come.  The parser keeps
 * the stream's state between the calls: what stands at the span's first byte (a member header, deflate data from a confirmed
 * bit on, a trailer), the last 32 KiB of the open member's text, its running CRC-32 and length.  Whole blocks are inflated
 * behind the carry, the text is cut at the last whole record and parsed as with kasa_bgzf_parse_append.
 *   *keepFrom     the byte of `bytes` from which the host sends again next time, more bytes behind it: where the last
 *                 confirmed block ends (a block the span's end cuts is not output).  0 with no text: no whole block ends
 *                 inside the span -- send a longer one.  A span of KASA_GZIP_SPAN_LIMIT bytes with no whole block is
 *                 KASA_INFLATE_SPAN (16 MiB: 250 times the largest block zlib writes, 256 MiB of symbols on the device).
 *   final         the file ends with the span: a member that does not end in it is KASA_INFLATE_TRUNCATED / _CUT.
 *   *parsable = 0 pool, carry and stream state are as before the call; KASA_PARSE_INFLATE: the stream is malformed --
 *                 kasa_gzip_parse_status gives the KASA_INFLATE_* code and the member's index in the FILE, and in stats8 (when
 *                 not NULL) the chunk statistics of kasa_gzip_inflate summed over the calls (rounds: the most one stream took).
 * kasa_gzip_parse_ms is kasa_bgzf_parse_ms (one counter).  KASA_GUNZIP_CHUNK in the environment: the chunk size in bytes. */
#define KASA_GZIP_SPAN_LIMIT (16u << 20)
int kasa_gzip_parse_append(kasa_parser *p, const void *bytes, uint64_t nBytes, int fasta, int final, uint64_t *nReadsAdded, int *parsable,
                           uint64_t *nTextBytes, uint64_t *keepFrom);
int kasa_gzip_parse_status(kasa_parser *p, int *code, uint64_t *member, uint64_t *stats8);
int kasa_gzip_parse_ms(kasa_parser *p, double *inflateMs);
int kasa_bgzf_parse_ms(kasa_parser *p, double *inflateMs);
/* Paired-end input (-1 <file> -2 <file>): TWO pools on one device, file 1 parsed into `first`, file 2 into `second`; pooled
 * read r of the one and pooled read r of the other are the mates of pair r.  The pools need not hold the same number of
 * reads: the one that ran ahead keeps its surplus.  Pairs come out in the form kasa_batch_upload_segments takes:
 *   bases    mate1(0) mate2(0) mate1(1) mate2(1) ..., untouched
 *   off      [2 n + 1] over the sequences (sequence s belongs to read s >> 1)
 *   names    name1(r) name2(r) back to back (each ends in its one space), with nameOff[n + 1]
 *   lengths  lengths1[r] + lengths2[r]
 * made on the device from the pools' running offsets in closed form (no scan) and ONE pass over the letters.
 *   kasa_pair_take   the first nPairs reads of both pools become ctx's batch of nPairs reads in 2 nPairs sequences and leave
 *                    the pools.  The letters are gathered straight into the context's own buffer (the pools' memory is
 *                    reused by their next append) and the context goes on as kasa_batch_upload_segments does.  Read-backs:
 *                    32 bytes per pool for the ends, the 8-byte k-mer count.  The call returns with the stream idle.  Both
 *                    heads advance together, or -- when the call fails -- neither.  nPairs = 0 gives an empty batch.
 *                    KASA_E_ARG, pools untouched: a pool holds fewer than nPairs reads, first == second, the pools or the
 *                    context lie on different devices, a pointer is NULL.
 *   kasa_pair_fetch  pairs [firstPair, firstPair + nPairs) in that form to host memory; any output pointer may be NULL; off
 *                    and nameOff are rebased to the first pair.  The pools stay as they are. */
int kasa_pair_take(kasa_parser *first, kasa_parser *second, kasa_ctx *ctx, uint64_t nPairs);
int kasa_pair_fetch(kasa_parser *first, kasa_parser *second, uint64_t firstPair, uint64_t nPairs, uint32_t *lengths, uint64_t *nameOff, char *names,
                    int64_t *off, uint8_t *bases);
/* --filter on the device (--device-filter): every read is written back to one of two files, so the pool can keep the reads'
 * RECORD TEXT: every non-empty line of the record (from its header line up to the next header or the chunk's end), each followed
 * by one line feed -- what the host driver's filterReads writes for the read.  A '\r' stays part of its line (a line that is only
 * "\r" is not empty), a last line without a line feed gets one; FASTQ records are their four lines, FASTA drops the empty ones.
 * (The two pool calls are named kasa_pool_*: kasa_parse_* stays the parser's surface as it was.)
 *   kasa_pool_keep_records   keep != 0: from now on every append (kasa_parse_append, kasa_bgzf_parse_append) also writes the
 *                             records and running 64-bit recOff[nReads + 1] behind the pool's end, under the same rule as the
 *                             other arrays (a refused chunk leaves them as they were); they are compacted with the pool, and
 *                             kasa_parse_take gives the context its own device-to-device copy of the taken reads' records with
 *                             offsets from 0, valid until the batch's last call.  keep = 0 (how a pool starts): no extra kernel
 *                             runs and no extra memory is taken.  KASA_E_STATE unless the pool is empty and nothing is carried.
 *                             kasa_pair_take / kasa_pair_fetch do not hand records on.
 *   kasa_pool_fetch_records  test tap: records and recOff of reads [first, first + n), rebased to `first`; either pointer may be
 *                             NULL; KASA_E_STATE when the pool keeps no records.
 *   kasa_batch_filter         after kasa_parse_take from such a pool: the batch's records split by flag, in the reads' order.
 *                             side 0: clean (flag 0), side 1: contaminants.  contaminated: nReads host bytes, or NULL for the
 *                             flags kasa_batch_text left on the device (a host array is what a driver has when kasa_batch_rank
 *                             left reads to the host, or when it wrote the rows itself).  sides: bit mask of the sides wanted (bit
 *                             0 clean, bit 1 contaminants); a side that is not wanted costs nothing and gives 0 and 0.
 *                             gzip != 0: each wanted side's text becomes a BGZF stream by the kernels of kasa_batch_bgzf in the
 *                             context's code (kasa_ctx_set_bgzf_code), without end-of-file block; nBytes is then the stream's
 *                             length.  nReads[side]: reads of that side.  An empty batch or side gives 0 and 0.  KASA_E_STATE:
 *                             the batch has no records (kasa_batch_upload*, kasa_pair_take), or contaminated is NULL and there
 *                             is no text of this batch.  One lane per read for the sizes, two running sums (flagged reads and
 *                             flagged bytes: the clean side's follow from recOff), one lane per read for the sides' lists, and
 *                             the 64-bit gather of kasa_pair_take split by output bytes; no atomics.
 *   kasa_batch_filter_fetch_range  dst[nBytes] = side's text (or stream) [offset, offset + nBytes).
 *   kasa_filter_split         test tap, host to host, the same kernels: one side of nReads records as plain text.  *nOut is the
 *                             side's size even when it exceeds cap (then KASA_E_LIMIT and nothing is written). */
int kasa_pool_keep_records(kasa_parser *p, int keep);
int kasa_pool_fetch_records(kasa_parser *p, uint64_t first, uint64_t n, uint64_t *recOff, char *records);
int kasa_batch_filter(kasa_ctx *ctx, const uint8_t *contaminated, unsigned sides, int gzip, uint64_t nBytes[2], uint64_t nReads[2]);
int kasa_batch_filter_fetch_range(kasa_ctx *ctx, int side, void *dst, uint64_t offset, uint64_t nBytes);
int kasa_filter_split(int device, const char *records, const uint64_t *recOff, uint64_t nReads, const uint8_t *flags, int side, char *out, uint64_t cap,
                      uint64_t *nOut, uint64_t *nReadsOut);
void kasa_parse_destroy(kasa_parser *p);

/* ---- an index larger than device memory: partitions come and go in slots (the reference streams its
 *      index from disk, Compare.hpp:286-318).  The index is cut between `_trie` entries as for kasa_batch_slice_starts; a
 *      slot of the pager is a kasa_index like any other, loaded again and again into the same device memory.
 *   kasa_index_pager_create  nSlots (>= 1) slots for partitions of at most maxRecords records of recordBytes (12, 20 or 6: as
 *                            kasa_index_create) -- keys, dense taxa, meta and a prefix table each --, one set of load
 *                            transients (raw records, the taxon sort's arrays, rocPRIM scratch, the trie arrays) and one
 *                            stream of the pager's own; the content's tax IDs go up once.  Nothing is allocated afterwards.
 *   kasa_index_pager_load    copies `records` (host memory of any kind, e.g. the mapped file) up and prepares the slot on the
 *                            pager's stream; returns when the slot is ready and the stream idle (overlap comes from a host
 *                            thread of the caller's).  A slot that already holds partitionId: nothing happens, a hit is
 *                            counted.  Refusals are kasa_index_create's, with its messages (unsorted or duplicate records, key
 *                            bits beyond the width, an unknown tax ID, a trie that does not describe the records), plus
 *                            KASA_E_LIMIT for nRecords > maxRecords; a refusal leaves the slot empty.  KASA_E_STATE while a
 *                            context is bound to the slot.
 *   kasa_index_pager_index   the slot as an index; KASA_E_STATE when it is empty.  Valid until the pager is destroyed; its
 *                            contents change with the next load into the slot.
 *   kasa_index_pager_stats   out[0..7] = loads, hits, bytes copied, copy us, prepare us, refused loads, device bytes of the
 *                            pager, 1 when the prepare kernel searches the tax-ID table in LDS.
 *   kasa_index_pager_tile    records a workgroup of the prepare kernel takes; most taxa whose table it searches in LDS.
 *   kasa_ctx_set_index       the context works on another index of the same device, key width and number of taxa (else
 *                            KASA_E_ARG) from its next batch on; its profile stays.  A pager counts the contexts bound to each of
 *                            its slots (kasa_ctx_create, kasa_ctx_set_index); rebinding or destroying the context releases it.
 *   kasa_batch_pool_keep     the owner of a sorted batch copies a grouped slice's pool into a buffer of its own and returns the
 *                            copy's place, valid until kasa_batch_records_import_device; the next kasa_batch_sort_and_range
 *                            clears the buffers.  (A worker that takes the next slice overwrites its pool.)
 *   kasa_index_fetch         test tap: one array of an index (`what` below) to host memory; bytes must be the array's size
 *                            (records x 8 or 16, x 4, x 1 or 2, 2^tb x 4, and 4 for tb itself as int32). */
typedef struct kasa_index_pager kasa_index_pager;
enum { KASA_INDEX_KEYS = 0, KASA_INDEX_TAXA = 1, KASA_INDEX_META = 2, KASA_INDEX_TABLE = 3, KASA_INDEX_TABLE_BITS = 4 };
int kasa_index_pager_create(int device, uint64_t maxRecords, int recordBytes, uint32_t nSlots, const uint32_t *taxIds, uint32_t nTaxa,
                            kasa_index_pager **out);
int kasa_index_pager_load(kasa_index_pager *pager, uint32_t slot, uint64_t partitionId, const void *records, uint64_t nRecords,
                          const uint32_t *triePrefix, const uint64_t *trieCount, uint64_t nTrie);
int kasa_index_pager_index(kasa_index_pager *pager, uint32_t slot, const kasa_index **ix);
int kasa_index_pager_stats(kasa_index_pager *pager, uint64_t out[8]);
int kasa_index_pager_tile(uint32_t *tileRecords, uint32_t *ldsTaxa);
int kasa_index_pager_destroy(kasa_index_pager *pager);
int kasa_ctx_set_index(kasa_ctx *ctx, const kasa_index *ix);
int kasa_batch_pool_keep(kasa_ctx *owner, const uint32_t *poolDev, uint64_t nPoolWords, const uint32_t **keptDev);
int kasa_index_fetch(const kasa_index *ix, int what, void *out, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif
