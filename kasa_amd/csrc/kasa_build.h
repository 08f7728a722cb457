// kasa_build.h -- `kASA build` on the device behind kasa_build_* of include/kasa_hip.h: a database's sequences -> the sorted,
// unique (k-mer, tax ID) records of the index file, its `_trie` and the `_f.txt` frequencies.
//
// Reference: in-RAM bricks + STXXL temporary files + a k-way merge (source/modes/Build.hpp:305-477, Read.hpp:2928-3176),
// the trie (Trie.hpp:365-394) and the frequency table (kASA.hpp:449-575).  Here:
//   brick   : sequences as the host hands them over, cut between sequences at maxPairs (pairs = what the encoder emits).
//             The host stages a brick and uploads its sequences ORDERED BY TAXON RANK (the rank of the tax ID among the
//             content file's sorted IDs, < 2^22): the encoder writes a sequence's pairs at the sequence's place, so the pairs
//             of a brick arrive ordered by rank, and ONE stable radix sort by k-mer leaves them ordered by (k-mer, rank) --
//             no passes over the rank and no wider composite key.                                   [encode_kernel, pass_kernel]
//   unique  : neighbour compare, running sum (rocPRIM), scatter: the brick's sorted run, kept in device memory  [bld_flag/scatter]
//   merge   : runs merged pairwise by merge path; a duplicate between two runs meets its twin as a neighbour and is dropped
//             in the same kernel (count, running sum, write)                                          [bld_merge_kernel]
//   emit    : file records {u64, u32 taxid} / {u64 lo, u64 hi, u32 taxid}, the trie's runs of 30-bit prefixes, a
//             [rank][trailing '^' letters] histogram turned into the frequency rows by a running sum   [bld_emit/trie/freq]
// Counts and offsets are 64-bit throughout; a single radix sort (one brick) holds fewer than 2^32 pairs.
#pragma once
#include <memory>
#include "kasa_spill_plan.h"

namespace kasa_build_impl {

static constexpr int MERGE_ITEMS = 8;                  // merged outputs per thread (one merge-path search each)
static constexpr int FREQ_LDS_CELLS = 16384;           // u32 histogram cells privatised in LDS (64 KiB)

template <class Key> __device__ __forceinline__ bool pair_less(Key ka, uint32_t ra, Key kb, uint32_t rb) { return ka < kb || (ka == kb && ra < rb); }

// a letter '_' (31: a codon with a base other than ACGT) -- DNA builds drop the k-mers that contain one (Read.hpp:2008-2066, "if a
// character is 'illegal' then don't save the kMer containing it"); amino-acid builds keep every k-mer (Read.hpp:2256-2266)
template <class Key> __device__ __forceinline__ bool has_illegal(Key x)
{
    return ((x & (x >> 1) & (x >> 2) & (x >> 3) & (x >> 4)) & field_repeat<Key>(1u)) != (Key)0;
}
// f[i] = pair i is kept: it differs from pair i - 1 (and, dropIllegal, has no '_'); the running sum turns flags into places
template <class Key>
__device__ __forceinline__ bool keep_pair(const Key *__restrict__ k, const uint32_t *__restrict__ v, uint64_t i, bool dropIllegal)
{
    return (i == 0 || k[i] != k[i - 1] || v[i] != v[i - 1]) && !(dropIllegal && has_illegal<Key>(k[i]));
}
template <class Key>
__global__ void bld_flag_kernel(const Key *__restrict__ k, const uint32_t *__restrict__ v, uint64_t n, int dropIllegal, uint32_t *__restrict__ f)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        f[i] = keep_pair<Key>(k, v, i, dropIllegal != 0) ? 1u : 0u;
}
template <class Key>
__global__ void bld_scatter_kernel(const Key *__restrict__ k, const uint32_t *__restrict__ v, uint64_t n, int dropIllegal, const uint32_t *__restrict__ pos,
                                   Key *__restrict__ ko, uint32_t *__restrict__ vo)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (keep_pair<Key>(k, v, i, dropIllegal != 0)) { ko[pos[i]] = k[i]; vo[pos[i]] = v[i]; }
}
// k-mers the host made (sequences of 1-8 letters, below): pair j goes to slot pos[j] of the brick, pos[j] < n
template <class Key>
__global__ void bld_place_kernel(const uint64_t *__restrict__ pos, const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi,
                                 const uint32_t *__restrict__ rank, uint64_t m, Key *__restrict__ k, uint32_t *__restrict__ v)
{
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x) {
        Key x = (Key)lo[j];
        if constexpr (sizeof(Key) > 8) x |= (Key)hi[j] << 64;
        k[pos[j]] = x; v[pos[j]] = rank[j];
    }
}

// Merge path over two sorted unique runs A, B: thread t owns merged outputs [t * ITEMS, (t + 1) * ITEMS), finds where that
// diagonal crosses the runs by binary search (ties: A first) and merges ITEMS steps.  WRITE = false: count the outputs that
// differ from their predecessor; WRITE = true: write them at base[t].  Bounds: reads A[0, nA), B[0, nB); writes
// out[base[t], base[t] + count[t]) with base the running sum of the counts, so inside [0, nA + nB).
template <class Key, bool WRITE>
__global__ __launch_bounds__(256) void bld_merge_kernel(const Key *__restrict__ ka, const uint32_t *__restrict__ va, uint64_t nA,
                                                        const Key *__restrict__ kb, const uint32_t *__restrict__ vb, uint64_t nB,
                                                        uint64_t *__restrict__ cnt, Key *__restrict__ ko, uint32_t *__restrict__ vo)
{
    const uint64_t nT = (nA + nB + MERGE_ITEMS - 1) / MERGE_ITEMS;
    for (uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; t < nT; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t d = t * MERGE_ITEMS;
        uint64_t lo = d > nB ? d - nB : 0, hi = d < nA ? d : nA;
        while (lo < hi) {                                              // first a in [lo, hi] with A[a] > B[d - 1 - a]
            const uint64_t mid = (lo + hi) >> 1;
            if (!pair_less<Key>(kb[d - 1 - mid], vb[d - 1 - mid], ka[mid], va[mid])) lo = mid + 1; else hi = mid;
        }
        uint64_t a = lo, b = d - lo;
        bool havePrev = false;
        Key pk = 0; uint32_t pv = 0;                                   // the merged output before this thread's first
        if (a > 0) { pk = ka[a - 1]; pv = va[a - 1]; havePrev = true; }
        if (b > 0 && (!havePrev || pair_less<Key>(pk, pv, kb[b - 1], vb[b - 1]))) { pk = kb[b - 1]; pv = vb[b - 1]; havePrev = true; }
        uint64_t w = WRITE ? cnt[t] : 0;
        uint32_t c = 0;
        for (int s = 0; s < MERGE_ITEMS && a + b < nA + nB; ++s) {
            Key k; uint32_t v;
            if (b >= nB || (a < nA && !pair_less<Key>(kb[b], vb[b], ka[a], va[a]))) { k = ka[a]; v = va[a]; ++a; }
            else { k = kb[b]; v = vb[b]; ++b; }
            if (!havePrev || k != pk || v != pv) {
                if (WRITE) { ko[w] = k; vo[w] = v; ++w; }
                ++c;
            }
            pk = k; pv = v; havePrev = true;
        }
        if (!WRITE) cnt[t] = c;
    }
}

// records in the file layout: 12 bytes {u64 kmer, u32 taxid} or 20 bytes {u64 lo, u64 hi, u32 taxid}, written as 32-bit words
// (a record starts at a multiple of 4 bytes).  Writes rec[0, n * bytes).
template <class Key>
__global__ void bld_emit_kernel(const Key *__restrict__ k, const uint32_t *__restrict__ rank, uint64_t n, const uint32_t *__restrict__ idOfRank,
                                uint32_t *__restrict__ rec)
{
    constexpr int W = sizeof(Key) / 4 + 1;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const Key x = k[i];
        uint32_t *r = rec + i * W;
#pragma unroll
        for (int j = 0; j < W - 1; ++j) r[j] = (uint32_t)(x >> (32 * j));
        r[W - 1] = idOfRank[rank[i]];
    }
}

// trie (Trie.hpp:365-394): where the top 30 bits (6 letters) change.  f[i] = 1 at the first key of a prefix.
template <class Key>
__global__ void bld_trie_flag_kernel(const Key *__restrict__ k, uint64_t n, int shift, uint32_t *__restrict__ f)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        f[i] = (i == 0 || (uint32_t)(k[i] >> shift) != (uint32_t)(k[i - 1] >> shift)) ? 1u : 0u;
}
template <class Key>
__global__ void bld_trie_scatter_kernel(const Key *__restrict__ k, uint64_t n, int shift, const uint64_t *__restrict__ pos,
                                        uint64_t *__restrict__ first, uint32_t *__restrict__ prefix)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t p = (uint32_t)(k[i] >> shift);
        if (i == 0 || p != (uint32_t)(k[i - 1] >> shift)) { first[pos[i]] = i; prefix[pos[i]] = p; }
    }
}
// first[j] (the first key of prefix j) -> count[j] = first[j + 1] - first[j]
__global__ void bld_trie_count_kernel(const uint64_t *__restrict__ first, uint64_t m, uint64_t n, uint64_t *__restrict__ count)
{
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < m; j += (uint64_t)gridDim.x * blockDim.x)
        count[j] = (j + 1 < m ? first[j + 1] : n) - first[j];
}

// frequencies (kASA.hpp:517-526): freq[tax][j] = unique entries whose letter j, counted from the right, is not '^' (30).
// The padding the encoder writes is a trailing run of '^', so an entry adds one to hist[rank][t], t = its trailing '^'
// letters, and freq[rank][j] = sum of hist[rank][0..j].  An entry with a '^' elsewhere (an input letter that encodes to 30)
// adds to extra[rank][j] letter by letter.  LDS: the histogram of all ranks when nRank * (K + 1) <= FREQ_LDS_CELLS.
template <class Key, bool LDS>
__global__ __launch_bounds__(256) void bld_freq_kernel(const Key *__restrict__ k, const uint32_t *__restrict__ rank, uint64_t n, uint32_t nRank,
                                                       unsigned long long *__restrict__ hist, unsigned long long *__restrict__ extra)
{
    constexpr int KL = KeyTraits<Key>::LETTERS;
    __shared__ uint32_t sh[LDS ? FREQ_LDS_CELLS : 1];
    const uint32_t cells = nRank * (uint32_t)(KL + 1);
    if (LDS) { for (uint32_t i = threadIdx.x; i < cells; i += blockDim.x) sh[i] = 0u; __syncthreads(); }
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const Key x = k[i];
        const uint32_t r = rank[i];
        int t = 0;
        while (t < KL && (uint32_t)((x >> (5 * t)) & 31) == 30u) ++t;
        bool inner = false;
        for (int j = t; j < KL; ++j) inner |= (uint32_t)((x >> (5 * j)) & 31) == 30u;
        if (!inner) {
            if (LDS) atomicAdd(&sh[r * (KL + 1) + t], 1u);
            else atomicAdd(&hist[(uint64_t)r * (KL + 1) + t], 1ull);
        } else {
            for (int j = t; j < KL; ++j)
                if ((uint32_t)((x >> (5 * j)) & 31) != 30u) atomicAdd(&extra[(uint64_t)r * KL + j], 1ull);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < cells; i += blockDim.x) if (sh[i]) atomicAdd(&hist[i], (unsigned long long)sh[i]);
    }
}
__global__ void bld_freq_final_kernel(const unsigned long long *__restrict__ hist, const unsigned long long *__restrict__ extra, uint32_t nRank, int KL,
                                      uint64_t *__restrict__ freq)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nRank) return;
    uint64_t run = 0;
    for (int j = 0; j < KL; ++j) { run += hist[(uint64_t)r * (KL + 1) + j]; freq[(uint64_t)r * KL + j] = run + extra[(uint64_t)r * KL + j]; }
}

static inline unsigned grid_for(uint64_t n, unsigned threads = 256, unsigned cap = 8192)
{
    const uint64_t b = (n + threads - 1) / threads;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(b, cap));
}

} // namespace kasa_build_impl

struct kasa_builder {
    int device = 0, K = 12, frames = 3;
    bool wide = false;
    // Where the build stands -- what every entry point checks first.  A finish that fails leaves ADDING.
    //   ADDING  add, add_index, drop_taxa, shrink and set_resident are taken
    //   SLABS   kasa_build_finish_begin is done; kasa_build_slab and fetch_slab hand the slabs out, slabNext is the next one
    //   DONE    kasa_build_finish_end is done (kasa_build_finish is begin + every slab + end)
    enum State { ADDING, SLABS, DONE } state = ADDING;
    // where the runs live: b->runs on the device, or (spilled) hostRuns, where every new run follows them
    bool spilled = false;
    // where the finished records and trie live, from SLABS on: all in rec / triePrefix / trieCount; the current slab's there and
    // no others; all in hRec / hTriePrefix / hTrieCount
    enum Records { ON_DEVICE, BY_SLAB, GATHERED } records = ON_DEVICE;
    // what was called: kasa_build_add; an edit call (add_index, drop_taxa, shrink); add_index in the middle of a run
    // (idxRuns.back() holds [0, loadNext) of loadTotal records)
    bool added = false, edited = false, loading = false;
    // The combinations that occur:
    //   spilled  records                                         edited, loading, halved
    //   false    ON_DEVICE: one slab, made by finish_begin        any: the edit calls refuse a budget and spilled runs
    //   true     BY_SLAB, or GATHERED after kasa_build_finish     never: set_resident refuses an edited builder, which never spills
    hipStream_t stream = nullptr;
    uint64_t maxPairs = 0;
    std::vector<uint32_t> ids;             // content tax IDs sorted ascending, unique: rank -> tax ID
    std::vector<uint32_t> rowRank;         // content row -> rank (~0u: a later row repeating an earlier row's tax ID)
    DevBuf lut, idOfRank;
    // the brick being staged on the host
    std::vector<uint8_t> hBases;
    std::vector<int64_t> hOff{0};
    std::vector<uint32_t> hRank;
    std::vector<uint64_t> hPairs;
    uint64_t stagedPairs = 0;
    int stagedProtein = -1;
    struct Tiny { uint64_t seq, w, lo, hi; };  // a k-mer of a very short sequence, made on the host (kasa_build_add)
    std::vector<Tiny> hTiny;
    uint8_t hostLut[366];
    // brick buffers
    DevBuf dBases, dBaseOff, dSeqOff, dSeqRank, dLong, kA, vA, kB, vB, flags, scanTmp, sortTmp;
    struct Run { DevBuf k, v; uint64_t n = 0; };
    std::vector<Run> runs;
    // result
    Run result;
    DevBuf rec, trieFirst, triePrefix, trieCount, freqR;
    uint64_t nTrie = 0;
    // stats: pairs in, bricks, merges, records out, ms encode / sort+unique / merge / emit
    uint64_t pairsIn = 0, bricks = 0, merges = 0;
    double ms[4] = {0, 0, 0, 0};
    // editing an existing index (kasa_edit.h): its runs, the taxa to drop, the shrink strategy
    std::vector<Run> idxRuns;
    uint64_t loadNext = 0, loadTotal = 0;
    DevBuf loadStage, loadErr;
    std::vector<uint8_t> dropRank;         // rank -> dropped (kasa_build_drop_taxa); empty: nothing dropped
    int shrinkStrategy = 0;                // 0: none, 1: every n-th of a taxon, 2: halved, 3: entropy
    float shrinkP = 0.f;
    bool halved = false;                   // set by the finish of shrink strategy 2: 6-byte records, and freqR holds the frequencies of the full index
    uint64_t indexIn = 0, droppedDelete = 0, droppedShrink = 0;
    double msEdit = 0;                     // device ms of the loads and the filters
    // building an index larger than device memory (kasa_spill.h): runs in host memory, merged and emitted in key-range slabs
    uint64_t resident = 0;                 // kasa_build_set_resident: the most input records of a slab (0: sized by the device)
    std::vector<kasa_spill_plan::HostRun> hostRuns;
    kasa_spill_plan::Plan plan;
    uint64_t slabNext = 0, totalRec = 0, totalTrie = 0;
    std::vector<uint8_t> hRec;             // records = GATHERED: the records and trie entries of all slabs
    std::vector<uint32_t> hTriePrefix;
    std::vector<uint64_t> hTrieCount;
    DevBuf freqHist, freqExtra;            // the frequency histograms, kept from the first slab to the last
    uint64_t spillRuns = 0, spillRecords = 0;
    double usUp = 0, usDown = 0;           // host microseconds of the copies host -> device, device -> host
    int keyBytes() const { return wide ? 16 : 8; }
    int recBytes() const { return halved ? 6 : (wide ? 20 : 12); }
    uint64_t nSlabs() const { return spilled ? plan.slabs.size() : 1; }
};

namespace kasa_build_impl {

// kasa_edit.h: the index runs' merges and the filters after the brick merges; the 6-byte records of a halved index
template <class Key> static int edit_finish(kasa_builder *b);
template <class Key> static int edit_emit_halved(kasa_builder *b, const Key *k, const uint32_t *v, uint64_t n);
// kasa_spill.h: a new run joins the spilled ones (nothing for a builder that does not spill); begin + every slab + end in one call
template <class Key> static int spill_after_brick(kasa_builder *b);
template <class Key> static int finish_all(kasa_builder *b, uint64_t *nRecords, uint64_t *nTrie);

// elapsed device time of a stage: events around it, read after the stream has drained
struct StageClock {
    hipEvent_t a = nullptr, b = nullptr;
    double *acc;
    hipStream_t s;
    StageClock(double *acc_, hipStream_t s_) : acc(acc_), s(s_) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, s); }
    void stop() { (void)hipEventRecord(b, s); }
    ~StageClock()
    {
        float t = 0.f;
        if (hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&t, a, b) == hipSuccess) *acc += t;
        (void)hipGetLastError();
        (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    }
};

template <class Key>
static int unique_into(kasa_builder *b, Key *k, uint32_t *v, uint64_t n, int dropIllegal, kasa_builder::Run &out)
{
    int rc;
    if ((rc = b->flags.reserve(n * 4 + 64))) return rc;
    uint32_t *f = b->flags.as<uint32_t>();
    bld_flag_kernel<Key><<<grid_for(n), 256, 0, b->stream>>>(k, v, n, dropIllegal, f);
    HIPCHK(hipGetLastError());
    uint32_t last = 0;
    if ((rc = fetch_async(b->stream, last, f + n - 1))) return rc;           // (the last flag, before the scan overwrites it)
    if ((rc = dev_exclusive_scan(b->scanTmp, b->stream, f, f, 0u, (size_t)n, rocprim::plus<uint32_t>()))) return rc;
    uint32_t lastPos = 0;
    if ((rc = fetch(b->stream, lastPos, f + n - 1))) return rc;
    const uint64_t nu = (uint64_t)lastPos + last;
    if ((rc = out.k.reserve(nu * sizeof(Key) + 64)) || (rc = out.v.reserve(nu * 4 + 64))) return rc;
    bld_scatter_kernel<Key><<<grid_for(n), 256, 0, b->stream>>>(k, v, n, dropIllegal, f, out.k.as<Key>(), out.v.as<uint32_t>());
    HIPCHK(hipGetLastError());
    out.n = nu;
    return KASA_OK;
}

// The staged brick: upload its sequences in rank order, encode (kLow = 1: every '^'-padded tail window), sort, unique -> a run.
template <class Key>
static int flush_brick(kasa_builder *b)
{
    const int64_t nSeq = (int64_t)b->hRank.size();
    auto reset = [&]() { b->hBases.clear(); b->hOff.assign(1, 0); b->hRank.clear(); b->hPairs.clear(); b->hTiny.clear(); b->stagedPairs = 0; };
    if (nSeq == 0 || b->stagedPairs == 0) { reset(); return KASA_OK; }
    const uint64_t n = b->stagedPairs;
    if (n >= 0xFFFFFFF0ull) return fail(KASA_E_LIMIT, "kasa_build: one sequence encodes to %llu pairs, more than one radix sort (2^32) holds", (unsigned long long)n);
    // order by rank (stable): the pairs of the brick then arrive ordered by rank
    std::vector<int64_t> order((size_t)nSeq);
    for (int64_t i = 0; i < nSeq; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return b->hRank[(size_t)x] < b->hRank[(size_t)y]; });
    bool inOrder = true;
    for (int64_t i = 0; i < nSeq && inOrder; ++i) inOrder = order[(size_t)i] == i;
    std::vector<uint8_t> ordered;
    std::vector<int64_t> off((size_t)nSeq + 1);
    std::vector<uint64_t> seqOff((size_t)nSeq + 1);
    std::vector<uint32_t> rank((size_t)nSeq);
    if (!inOrder) ordered.resize(b->hBases.size());
    off[0] = 0; seqOff[0] = 0;
    for (int64_t i = 0; i < nSeq; ++i) {
        const int64_t s = order[(size_t)i], len = b->hOff[(size_t)s + 1] - b->hOff[(size_t)s];
        if (!inOrder && len) memcpy(ordered.data() + off[(size_t)i], b->hBases.data() + b->hOff[(size_t)s], (size_t)len);
        off[(size_t)i + 1] = off[(size_t)i] + len;
        seqOff[(size_t)i + 1] = seqOff[(size_t)i] + b->hPairs[(size_t)s];
        rank[(size_t)i] = b->hRank[(size_t)s];
    }
    const uint8_t *bases = inOrder ? b->hBases.data() : ordered.data();
    const uint64_t nBases = (uint64_t)off[(size_t)nSeq];
    int rc;
    if ((rc = b->dBases.reserve(nBases + 64)) || (rc = b->dBaseOff.reserve(((size_t)nSeq + 1) * 8)) || (rc = b->dSeqOff.reserve(((size_t)nSeq + 1) * 8)) ||
        (rc = b->dSeqRank.reserve((size_t)nSeq * 4 + 64)) || (rc = b->dLong.reserve(((size_t)nSeq + 1) * 4 + 64)) ||
        (rc = b->kA.reserve(n * sizeof(Key) + 64)) || (rc = b->vA.reserve(n * 4 + 64)) || (rc = b->kB.reserve(n * sizeof(Key) + 64)) ||
        (rc = b->vB.reserve(n * 4 + 64)) || (rc = b->sortTmp.reserve(kasa_radix::scratch_bytes<Key>(n))))
        return rc;
    HIPCHK(hipMemcpyAsync(b->dBases.p, bases, nBases, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->dBaseOff.p, off.data(), ((size_t)nSeq + 1) * 8, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->dSeqOff.p, seqOff.data(), ((size_t)nSeq + 1) * 8, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->dSeqRank.p, rank.data(), (size_t)nSeq * 4, hipMemcpyHostToDevice, b->stream));
    const int mode = b->stagedProtein == 1 ? ENC_PROTEIN : (b->frames == 1 ? ENC_ONE : ENC_DNA);
    {
        StageClock clk(&b->ms[0], b->stream);
        // payload = seqRead[s] = the sequence's rank; sequences of ENC_LONG_MIN pairs and more: their chunks over all wavefronts
        const unsigned blocks = (unsigned)std::min<int64_t>((nSeq + ENC_WAVES - 1) / ENC_WAVES, 256 * 16);
        encode_kernel<Key><<<blocks, 64 * ENC_WAVES, 0, b->stream>>>(b->dBases.as<uint8_t>(), b->dBaseOff.as<int64_t>(), b->dSeqOff.as<uint64_t>(),
            b->dSeqRank.as<uint32_t>(), nSeq, 1, 1, mode, b->lut.as<uint8_t>(), b->kA.as<Key>(), b->vA.as<uint32_t>(), 0, nullptr, nullptr, (uint64_t)ENC_LONG_MIN);
        HIPCHK(hipGetLastError());
        uint32_t *nLong = b->dLong.as<uint32_t>(), *list = nLong + 1;
        HIPCHK(hipMemsetAsync(nLong, 0, 4, b->stream));
        enc_long_list_kernel<<<blocks_for((uint64_t)nSeq, 256), 256, 0, b->stream>>>(b->dSeqOff.as<uint64_t>(), nSeq, ENC_LONG_MIN, list, nLong);
        encode_kernel<Key, ENC_RANK_MAX, true><<<256 * 8, 64 * ENC_WAVES, 0, b->stream>>>(b->dBases.as<uint8_t>(), b->dBaseOff.as<int64_t>(), b->dSeqOff.as<uint64_t>(),
            b->dSeqRank.as<uint32_t>(), nSeq, 1, 1, mode, b->lut.as<uint8_t>(), b->kA.as<Key>(), b->vA.as<uint32_t>(), 0, list, nLong, (uint64_t)ENC_LONG_MIN);
        HIPCHK(hipGetLastError());
        if (!b->hTiny.empty()) {                                       // the host's k-mers of very short sequences, at their slots
            std::vector<int64_t> placeOf((size_t)nSeq);
            for (int64_t i = 0; i < nSeq; ++i) placeOf[(size_t)order[(size_t)i]] = i;
            const size_t m = b->hTiny.size();
            std::vector<uint64_t> tp(m), tl(m), th(m);
            std::vector<uint32_t> tr(m);
            for (size_t j = 0; j < m; ++j) {
                const kasa_builder::Tiny &t = b->hTiny[j];
                tp[j] = seqOff[(size_t)placeOf[(size_t)t.seq]] + t.w; tl[j] = t.lo; th[j] = t.hi; tr[j] = b->hRank[(size_t)t.seq];
            }
            DevBuf dt;
            if ((rc = dt.reserve(m * 28 + 64))) return rc;
            uint64_t *dp = dt.as<uint64_t>(), *dl = dp + m, *dh = dl + m;
            uint32_t *dr = reinterpret_cast<uint32_t *>(dh + m);
            HIPCHK(hipMemcpyAsync(dp, tp.data(), m * 8, hipMemcpyHostToDevice, b->stream));
            HIPCHK(hipMemcpyAsync(dl, tl.data(), m * 8, hipMemcpyHostToDevice, b->stream));
            HIPCHK(hipMemcpyAsync(dh, th.data(), m * 8, hipMemcpyHostToDevice, b->stream));
            HIPCHK(hipMemcpyAsync(dr, tr.data(), m * 4, hipMemcpyHostToDevice, b->stream));
            bld_place_kernel<Key><<<grid_for(m), 256, 0, b->stream>>>(dp, dl, dh, dr, m, b->kA.as<Key>(), b->vA.as<uint32_t>());
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(b->stream));                  // (the host vectors and `dt` go out of scope here)
        }
        clk.stop();
    }
    kasa_builder::Run run;
    {
        StageClock clk(&b->ms[1], b->stream);
        Key *kRes; uint32_t *vRes;
        HIPCHK(kasa_radix::sort_pairs<Key>(b->kA.as<Key>(), b->vA.as<uint32_t>(), b->kB.as<Key>(), b->vB.as<uint32_t>(), (uint32_t)n, 0,
                                           8 * ((KeyTraits<Key>::BITS + 7) / 8), b->sortTmp.p, b->stream, &kRes, &vRes));
        if ((rc = unique_into<Key>(b, kRes, vRes, n, mode != ENC_PROTEIN, run))) return rc;
        clk.stop();
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    b->runs.push_back(std::move(run));
    ++b->bricks;
    reset();
    return spill_after_brick<Key>(b);
}

template <class Key>
static int merge_two(kasa_builder *b, kasa_builder::Run &A, kasa_builder::Run &B, kasa_builder::Run &out)
{
    const uint64_t nOut = A.n + B.n, nT = (nOut + MERGE_ITEMS - 1) / MERGE_ITEMS;
    int rc;
    // what a merge needs beside the runs: its output and one count per thread
    const uint64_t need = nOut * (sizeof(Key) + 4) + (nT + 1) * 8 + 4096;
    size_t freeB = 0, totalB = 0;
    HIPCHK(hipMemGetInfo(&freeB, &totalB));
    if (need > freeB)
        return fail(KASA_E_LIMIT, "kasa_build_finish: merging two runs of %llu and %llu records needs %.2f GB of device memory beside the runs, %.2f GB are free "
                    "(the unique result plus one merge buffer must fit on the device)", (unsigned long long)A.n, (unsigned long long)B.n, need / 1e9, freeB / 1e9);
    DevBuf cnt;
    if ((rc = cnt.reserve((nT + 1) * 8))) return rc;
    uint64_t *c = cnt.as<uint64_t>();
    const unsigned g = grid_for(nT);
    bld_merge_kernel<Key, false><<<g, 256, 0, b->stream>>>(A.k.as<Key>(), A.v.as<uint32_t>(), A.n, B.k.as<Key>(), B.v.as<uint32_t>(), B.n, c, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(c + nT, 0, 8, b->stream));
    if ((rc = dev_exclusive_scan(b->scanTmp, b->stream, c, c, (uint64_t)0, (size_t)nT + 1, rocprim::plus<uint64_t>()))) return rc;
    uint64_t nu = 0;
    if ((rc = fetch(b->stream, nu, c + nT))) return rc;
    if ((rc = out.k.reserve(nu * sizeof(Key) + 64)) || (rc = out.v.reserve(nu * 4 + 64))) return rc;
    bld_merge_kernel<Key, true><<<g, 256, 0, b->stream>>>(A.k.as<Key>(), A.v.as<uint32_t>(), A.n, B.k.as<Key>(), B.v.as<uint32_t>(), B.n, c, out.k.as<Key>(), out.v.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));
    out.n = nu;
    ++b->merges;
    return KASA_OK;
}

// the frequency rows by rank into b->freqR in three steps: the histograms zeroed, the run (k, v, n) counted into them (any
// number of runs: the slabs of kasa_spill.h), the running sums
template <class Key>
static int freq_zero(kasa_builder *b)
{
    const uint32_t nRank = (uint32_t)b->ids.size();
    constexpr int KL = KeyTraits<Key>::LETTERS;
    int rc;
    if ((rc = b->freqR.reserve((size_t)nRank * KL * 8 + 64)) || (rc = b->freqHist.reserve((size_t)nRank * (KL + 1) * 8 + 64)) || (rc = b->freqExtra.reserve((size_t)nRank * KL * 8 + 64))) return rc;
    HIPCHK(hipMemsetAsync(b->freqHist.p, 0, (size_t)nRank * (KL + 1) * 8, b->stream));
    HIPCHK(hipMemsetAsync(b->freqExtra.p, 0, (size_t)nRank * KL * 8, b->stream));
    return KASA_OK;
}
template <class Key>
static int freq_accumulate(kasa_builder *b, const Key *k, const uint32_t *v, uint64_t n)
{
    const uint32_t nRank = (uint32_t)b->ids.size();
    constexpr int KL = KeyTraits<Key>::LETTERS;
    if (n) {
        if ((uint64_t)nRank * (KL + 1) <= (uint64_t)FREQ_LDS_CELLS)
            bld_freq_kernel<Key, true><<<grid_for(n, 256, 1024), 256, 0, b->stream>>>(k, v, n, nRank, b->freqHist.as<unsigned long long>(), b->freqExtra.as<unsigned long long>());
        else
            bld_freq_kernel<Key, false><<<grid_for(n, 256, 8192), 256, 0, b->stream>>>(k, v, n, nRank, b->freqHist.as<unsigned long long>(), b->freqExtra.as<unsigned long long>());
        HIPCHK(hipGetLastError());
    }
    return KASA_OK;
}
template <class Key>
static int freq_final(kasa_builder *b)
{
    const uint32_t nRank = (uint32_t)b->ids.size();
    constexpr int KL = KeyTraits<Key>::LETTERS;
    bld_freq_final_kernel<<<blocks_for(nRank, 256), 256, 0, b->stream>>>(b->freqHist.as<unsigned long long>(), b->freqExtra.as<unsigned long long>(), nRank, KL, b->freqR.as<uint64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));
    b->freqHist.release(); b->freqExtra.release();
    return KASA_OK;
}
// the runs merged pairwise, level by level, until one is left: every record takes part in log2(runs) merges.  When a merge fails
// the runs stay whole -- those merged so far and the rest -- and the caller may go on by slabs (kasa_spill.h).
template <class Key>
static int merge_runs(kasa_builder *b, std::vector<kasa_builder::Run> &runs)
{
    int rc;
    while (runs.size() > 1) {
        std::vector<kasa_builder::Run> next;
        for (size_t i = 0; i + 1 < runs.size(); i += 2) {
            kasa_builder::Run m;
            if ((rc = merge_two<Key>(b, runs[i], runs[i + 1], m))) {
                for (size_t j = i; j < runs.size(); ++j) next.push_back(std::move(runs[j]));
                runs.swap(next);
                return rc;
            }
            runs[i].k.release(); runs[i].v.release(); runs[i + 1].k.release(); runs[i + 1].v.release();
            next.push_back(std::move(m));
        }
        if (runs.size() % 2) next.push_back(std::move(runs.back()));
        runs.swap(next);
    }
    return KASA_OK;
}

// flags f[0, n), n > 0 -> pos[i] = how many of f[0, i) are set, `kept` = how many of all n: where each flagged item goes, in 64 bits
static int flag_places(kasa_builder *b, const uint32_t *f, uint64_t n, uint64_t *pos, uint64_t &kept)
{
    int rc;
    rocprim::transform_iterator<const uint32_t *, rocprim::identity<uint64_t>, uint64_t> fin(f, rocprim::identity<uint64_t>());
    if ((rc = dev_exclusive_scan(b->scanTmp, b->stream, fin, pos, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>()))) return rc;
    uint64_t lastPos = 0; uint32_t lastF = 0;
    if ((rc = fetch_async(b->stream, lastPos, pos + n - 1)) || (rc = fetch(b->stream, lastF, f + n - 1))) return rc;
    kept = lastPos + lastF;
    return KASA_OK;
}

// b->result -> the file records in b->rec and the trie in b->triePrefix / trieCount (b->nTrie entries)
template <class Key>
static int emit_result(kasa_builder *b)
{
    int rc;
    const uint64_t n = b->result.n;
    const Key *k = b->result.k.as<Key>();
    const uint32_t *v = b->result.v.as<uint32_t>();
    constexpr int KL = KeyTraits<Key>::LETTERS;
    if ((rc = b->rec.reserve(n * (uint64_t)b->recBytes() + 64))) return rc;
    if (n) {
        if (b->halved) { if ((rc = edit_emit_halved<Key>(b, k, v, n))) return rc; }
        else bld_emit_kernel<Key><<<grid_for(n), 256, 0, b->stream>>>(k, v, n, b->idOfRank.as<uint32_t>(), b->rec.as<uint32_t>());
        HIPCHK(hipGetLastError());
        // trie
        const int shift = 5 * (KL - RANGE_LETTERS);
        DevBuf pos;
        if ((rc = pos.reserve((n + 1) * 8)) || (rc = b->flags.reserve(n * 4 + 64))) return rc;
        uint32_t *f = b->flags.as<uint32_t>();
        uint64_t *p = pos.as<uint64_t>();
        bld_trie_flag_kernel<Key><<<grid_for(n), 256, 0, b->stream>>>(k, n, shift, f);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(p + n, 0, 8, b->stream));
        if ((rc = flag_places(b, f, n, p, b->nTrie))) return rc;
        if ((rc = b->trieFirst.reserve(b->nTrie * 8 + 64)) || (rc = b->triePrefix.reserve(b->nTrie * 4 + 64)) || (rc = b->trieCount.reserve(b->nTrie * 8 + 64))) return rc;
        bld_trie_scatter_kernel<Key><<<grid_for(n), 256, 0, b->stream>>>(k, n, shift, p, b->trieFirst.as<uint64_t>(), b->triePrefix.as<uint32_t>());
        bld_trie_count_kernel<<<grid_for(b->nTrie), 256, 0, b->stream>>>(b->trieFirst.as<uint64_t>(), b->nTrie, n, b->trieCount.as<uint64_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(b->stream));                      // (pos goes out of scope here)
    } else b->nTrie = 0;
    return KASA_OK;
}

// The tail of every slab -- of the only one, first = last = true, when the runs stayed on the device: b->result -> the file records
// and the trie of the slab, its share of the frequency histograms (zeroed before the first slab, summed up after the last one),
// the running totals.  b->result's keys and ranks are released, the records and the trie stay until the next slab.
template <class Key>
static int finish_slab(kasa_builder *b, bool first, bool last)
{
    int rc;
    {
        StageClock clk(&b->ms[3], b->stream);
        if ((rc = emit_result<Key>(b))) return rc;
        if (!b->halved) {                                              // (a halved index keeps the frequencies of the full one: edit_finish)
            if (first && (rc = freq_zero<Key>(b))) return rc;
            if ((rc = freq_accumulate<Key>(b, b->result.k.as<Key>(), b->result.v.as<uint32_t>(), b->result.n))) return rc;
            if (last && (rc = freq_final<Key>(b))) return rc;
        }
        clk.stop();
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    b->result.k.release(); b->result.v.release();
    b->totalRec += b->result.n; b->totalTrie += b->nTrie;
    return KASA_OK;
}

} // namespace kasa_build_impl

extern "C" void kasa_build_destroy(kasa_builder *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

static int build_create_impl(int device, int K, int frames, const uint8_t *codonLut, const uint32_t *taxIds, uint32_t nTaxa, uint64_t maxPairsPerBrick,
                             kasa_builder **out)
{
    if (!out) return fail(KASA_E_ARG, "kasa_build_create: out is NULL");
    *out = nullptr;
    if (K != 12 && K != 25) return fail(KASA_E_ARG, "kasa_build_create: K must be 12 (64-bit index) or 25 (128-bit index, --kH 25), got %d", K);
    if (frames != 1 && frames != 3) return fail(KASA_E_ARG, "kasa_build_create: frames must be 3, or 1 (--one), got %d", frames);
    if (!taxIds || nTaxa < 2) return fail(KASA_E_ARG, "kasa_build_create: content mapping missing");
    if (nTaxa >= (1u << 22)) return fail(KASA_E_LIMIT, "kasa_build_create: %u taxa exceed the 2^22 taxon indices an event record can name", nTaxa);
    int ndev = 0;
    kasa_device_count(&ndev);
    if (device < 0 || device >= ndev) return fail(KASA_E_HIP, "kasa_build_create: no HIP device %d (found %d)", device, ndev);
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<kasa_builder> b(new kasa_builder());
    b->device = device; b->K = K; b->frames = frames; b->wide = K == 25;
    b->ids.assign(taxIds, taxIds + nTaxa);
    std::sort(b->ids.begin(), b->ids.end());
    b->ids.erase(std::unique(b->ids.begin(), b->ids.end()), b->ids.end());
    b->rowRank.assign(nTaxa, ~0u);
    std::vector<bool> seen(b->ids.size(), false);
    for (uint32_t r = 0; r < nTaxa; ++r) {                            // the first row of a tax ID owns its frequencies (formats.dense_tax)
        const uint32_t rk = (uint32_t)(std::lower_bound(b->ids.begin(), b->ids.end(), taxIds[r]) - b->ids.begin());
        if (!seen[rk]) { seen[rk] = true; b->rowRank[r] = rk; }
    }
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) return fail(KASA_E_HIP, "hipStreamCreate failed");
    uint8_t lut[366];
    if (codonLut) memcpy(lut, codonLut, 366); else builtin_codon_table(lut);
    memcpy(b->hostLut, lut, 366);
    int rc;
    if ((rc = b->lut.reserve(512)) || (rc = b->idOfRank.reserve(b->ids.size() * 4 + 64))) return rc;
    HIPCHK(hipMemcpy(b->lut.p, lut, 366, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->idOfRank.p, b->ids.data(), b->ids.size() * 4, hipMemcpyHostToDevice));
    if (maxPairsPerBrick == 0) {
        // automatic: a brick (both sort buffers, flags, its run) takes at most an eighth of the free memory, the rest is left to the runs
        size_t freeB = 0, totalB = 0;
        HIPCHK(hipMemGetInfo(&freeB, &totalB));
        const uint64_t perPair = 2 * ((uint64_t)b->keyBytes() + 4) + 8 + (uint64_t)b->keyBytes() + 4;
        maxPairsPerBrick = std::max<uint64_t>(1u << 20, (uint64_t)freeB / 8 / perPair);
    }
    b->maxPairs = std::min<uint64_t>(maxPairsPerBrick, 0xF0000000ull);
    *out = b.release();
    return KASA_OK;
}

extern "C" int kasa_build_create(int device, int K, int frames, const uint8_t *codonLut, const uint32_t *taxIds, uint32_t nTaxa, uint64_t maxPairsPerBrick,
                                 kasa_builder **out)
{
    KASA_GUARDED(build_create_impl(device, K, frames, codonLut, taxIds, nTaxa, maxPairsPerBrick, out))
}

static int build_add_impl(kasa_builder *b, const uint8_t *bases, const int64_t *offsets, int64_t nSeq, const uint32_t *seqTaxId, int protein)
{
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->state != kasa_builder::ADDING) return fail(KASA_E_STATE, "kasa_build_add: the build is finished");
    if (nSeq < 0 || (nSeq > 0 && (!offsets || !bases || !seqTaxId))) return fail(KASA_E_ARG, "kasa_build_add: bad arguments");
    HIPCHK(hipSetDevice(b->device));
    const int mode = protein ? ENC_PROTEIN : (b->frames == 1 ? ENC_ONE : ENC_DNA);
    int rc;
    b->added = true;
    for (int64_t s = 0; s < nSeq; ++s) {
        const int64_t len = offsets[s + 1] - offsets[s];
        if (len < 0) return fail(KASA_E_ARG, "kasa_build_add: offsets are not ascending at sequence %lld", (long long)s);
        const auto it = std::lower_bound(b->ids.begin(), b->ids.end(), seqTaxId[s]);
        if (it == b->ids.end() || *it != seqTaxId[s]) return fail(KASA_E_ARG, "kasa_build_add: sequence %lld has tax ID %u, which the content file does not list", (long long)s, seqTaxId[s]);
        int64_t body, L, cnt = 0;
        if (len > 0) enc_geometry(mode, b->K, 1, len, body, L, cnt);
        // What the reference's build emits (Read.hpp:1991-2290: windows = length + marker - K letters + 1, no padding) is what the
        // encoder emits for kLow = 1, except for sequences of 1-2 letters (amino acids), 3-4 bases (three frames) or 3-8 bases
        // (--one): the read geometry the encoder follows pads those and emits nothing.  Their few k-mers are made here.
        const int64_t want = mode == ENC_PROTEIN ? len : (mode == ENC_ONE ? (len >= 3 ? len / 3 : 0) : (len >= 3 ? len - 2 : 0));
        const bool tiny = cnt == 0 && want > 0;
        if (tiny) cnt = want;
        if (cnt == 0) continue;
        // a brick ends between sequences: before the one that would overflow it, and where the alphabet changes
        if (b->stagedPairs && (b->stagedPairs + (uint64_t)cnt > b->maxPairs || b->stagedProtein != (protein ? 1 : 0))) {
            if ((rc = b->wide ? kasa_build_impl::flush_brick<key128>(b) : kasa_build_impl::flush_brick<uint64_t>(b))) return rc;
        }
        b->stagedProtein = protein ? 1 : 0;
        b->hBases.insert(b->hBases.end(), bases + offsets[s], bases + offsets[s + 1]);
        b->hOff.push_back((int64_t)b->hBases.size());
        b->hRank.push_back((uint32_t)(it - b->ids.begin()));
        b->hPairs.push_back((uint64_t)cnt);
        b->stagedPairs += (uint64_t)cnt;
        if (tiny) {
            const uint8_t *q = bases + offsets[s];
            auto code = [&](int64_t p) -> int {                            // the encoder's 3-bit codes: 4 = X (marker), 5 = Z
                if (p >= len) return 4;
                const uint8_t ch = q[p], up = ch & 0xDF;
                return (up == 'A' || up == 'C' || up == 'G' || up == 'T') ? (ch & 14) >> 1 : 5;
            };
            for (int64_t w = 0; w < cnt; ++w) {
                unsigned __int128 key = 0;
                for (int i = 0; i < b->K; ++i) {
                    unsigned letter;
                    if (mode == ENC_PROTEIN) {
                        const int64_t p = w + i;
                        letter = p < len ? ((q[p] == '*' ? (uint8_t)'[' : q[p]) & 31u) : 30u;   // padding '^' (Read.hpp:663-667)
                    } else {
                        const int64_t p = (mode == ENC_ONE ? 3 * w : w) + 3 * i;
                        letter = b->hostLut[code(p) * 64 + code(p + 1) * 8 + code(p + 2)];
                    }
                    key = (key << 5) | letter;
                }
                b->hTiny.push_back({(uint64_t)b->hRank.size() - 1, (uint64_t)w, (uint64_t)key, (uint64_t)(key >> 64)});
            }
        }
        b->pairsIn += (uint64_t)cnt;
    }
    return KASA_OK;
}

extern "C" int kasa_build_add(kasa_builder *b, const uint8_t *bases, const int64_t *offsets, int64_t nSeq, const uint32_t *seqTaxId, int protein)
{
    KASA_GUARDED(build_add_impl(b, bases, offsets, nSeq, seqTaxId, protein))
}

extern "C" int kasa_build_finish(kasa_builder *b, uint64_t *nRecords, uint64_t *nTrie)
{
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->state != kasa_builder::ADDING) return fail(KASA_E_STATE, "kasa_build_finish: called twice");
    HIPCHK(hipSetDevice(b->device));
    try { return b->wide ? kasa_build_impl::finish_all<key128>(b, nRecords, nTrie) : kasa_build_impl::finish_all<uint64_t>(b, nRecords, nTrie); }
    catch (const std::bad_alloc &) { return fail(KASA_E_NOMEM, "host allocation failed"); }
}

extern "C" int kasa_build_fetch_range(kasa_builder *b, uint64_t first, uint64_t count, void *records)
{
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->state == kasa_builder::ADDING) return fail(KASA_E_STATE, "kasa_build_fetch: kasa_build_finish first");
    if (first > b->result.n || count > b->result.n - first) return fail(KASA_E_ARG, "kasa_build_fetch_range: [%llu, +%llu) outside the %llu records",
                                                                         (unsigned long long)first, (unsigned long long)count, (unsigned long long)b->result.n);
    if (count && !records) return fail(KASA_E_ARG, "kasa_build_fetch_range: records is NULL");
    if (b->records != kasa_builder::ON_DEVICE) {                       // (kasa_spill.h: the slabs' records, kept by kasa_build_finish)
        if (b->state != kasa_builder::DONE || b->records != kasa_builder::GATHERED) return fail(KASA_E_STATE, "kasa_build_fetch_range: the records of a spilled build were handed out slab by slab (kasa_build_fetch_slab)");
        if (count) memcpy(records, b->hRec.data() + first * (uint64_t)b->recBytes(), count * (uint64_t)b->recBytes());
        return KASA_OK;
    }
    HIPCHK(hipSetDevice(b->device));
    if (count) HIPCHK(hipMemcpy(records, b->rec.as<uint8_t>() + first * (uint64_t)b->recBytes(), count * (uint64_t)b->recBytes(), hipMemcpyDeviceToHost));
    return KASA_OK;
}

extern "C" int kasa_build_fetch(kasa_builder *b, void *records, uint32_t *triePrefix, uint64_t *trieCount, uint64_t *freq)
{
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->state == kasa_builder::ADDING) return fail(KASA_E_STATE, "kasa_build_fetch: kasa_build_finish first");
    HIPCHK(hipSetDevice(b->device));
    if (b->records != kasa_builder::ON_DEVICE && b->state != kasa_builder::DONE) return fail(KASA_E_STATE, "kasa_build_fetch: kasa_build_finish_end first");
    if (records) { const int rc = kasa_build_fetch_range(b, 0, b->result.n, records); if (rc) return rc; }
    if (b->records != kasa_builder::ON_DEVICE) {                       // (kasa_spill.h: the slabs' trie entries, kept by kasa_build_finish)
        if ((triePrefix || trieCount) && b->records != kasa_builder::GATHERED) return fail(KASA_E_STATE, "kasa_build_fetch: the trie of a spilled build was handed out slab by slab (kasa_build_fetch_slab)");
        if (triePrefix && b->nTrie) memcpy(triePrefix, b->hTriePrefix.data(), b->nTrie * 4);
        if (trieCount && b->nTrie) memcpy(trieCount, b->hTrieCount.data(), b->nTrie * 8);
        triePrefix = nullptr; trieCount = nullptr;
    }
    if (triePrefix && b->nTrie) HIPCHK(hipMemcpy(triePrefix, b->triePrefix.p, b->nTrie * 4, hipMemcpyDeviceToHost));
    if (trieCount && b->nTrie) HIPCHK(hipMemcpy(trieCount, b->trieCount.p, b->nTrie * 8, hipMemcpyDeviceToHost));
    if (freq) {
        const size_t nR = b->ids.size(), KL = (size_t)b->K;
        std::vector<uint64_t> byRank(nR * KL);
        HIPCHK(hipMemcpy(byRank.data(), b->freqR.p, nR * KL * 8, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < b->rowRank.size(); ++r) {
            if (b->rowRank[r] == ~0u) std::fill(freq + r * KL, freq + (r + 1) * KL, (uint64_t)0);
            else memcpy(freq + r * KL, byRank.data() + (size_t)b->rowRank[r] * KL, KL * 8);
        }
    }
    return KASA_OK;
}

extern "C" int kasa_build_stats(kasa_builder *b, uint64_t *stats8)
{
    if (!b || !stats8) return fail(KASA_E_ARG, "kasa_build_stats: NULL argument");
    stats8[0] = b->pairsIn; stats8[1] = b->bricks; stats8[2] = b->merges; stats8[3] = b->result.n;
    for (int i = 0; i < 4; ++i) stats8[4 + i] = (uint64_t)(b->ms[i] * 1000.0 + 0.5);   // device microseconds per stage
    return KASA_OK;
}
