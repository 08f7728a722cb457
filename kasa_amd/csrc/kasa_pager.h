// kasa_pager.h -- partitions of an index larger than device memory come and go (include/kasa_hip.h, kasa_index_pager_*;
// DESIGN.md section 8r).  Included by kasa_hip.hip after the context: it uses kasa_index, kasa_ctx, DevBuf, the dev_*
// primitives, dup_level_kernel and lcp_letters as they are.
//
// A pager owns nSlots index slots of one size (keys, dense taxa, meta, prefix table for `maxRecords` records), ONE set of
// load transients and ONE stream.  kasa_index_pager_load copies a partition's records as they are on disk into the
// transients and prepares the slot from them on that stream; a slot is a kasa_index like any other, so every kernel of the
// batch reads it unchanged.  Nothing is allocated after kasa_index_pager_create.
//
// What runs beside the batch's kernels is page_prepare_kernel: kasa_index_create's five passes over the records
// (unpack, order check, dense taxa, lcpPrev, table marks) in one.
#pragma once

// ---- the pager's counter block -------------------------------------------------------------------------------------------
// 64 bytes of device memory the kernels are handed the address of; this struct is its map (as CtxCounters is the context's).
struct PagerCounters {
    uint32_t order;                    // records out of (kmer, taxid) order, equal to the one before, or with key bits beyond the width
    uint32_t unknownTax;               // records whose tax ID the content file does not know
    uint32_t badTix;                   // halved records whose taxon index is >= nTaxa
    uint32_t trie;                     // `_trie` entries that do not describe the records
    unsigned long long firstBadTix;    // the first of the badTix records (the refusal names it)
    uint32_t unused[10];
};
static constexpr size_t PAGER_COUNTER_BYTES = 64;
#define KASA_PCTR_AT(field, bytes) static_assert(offsetof(PagerCounters, field) == (bytes), "PagerCounters::" #field " moved: the kernels address it by this offset")
KASA_PCTR_AT(order, 0); KASA_PCTR_AT(unknownTax, 4); KASA_PCTR_AT(badTix, 8); KASA_PCTR_AT(trie, 12); KASA_PCTR_AT(firstBadTix, 16);
#undef KASA_PCTR_AT
static_assert(sizeof(PagerCounters) == PAGER_COUNTER_BYTES, "the counter block is allocated once, with the pager");

// ---- the prepare kernel ---------------------------------------------------------------------------------------------------
static constexpr int PAGE_TILE = 1024;             // raw records per workgroup
static constexpr int PAGE_THREADS = 256;
static constexpr int PAGE_ITEMS = PAGE_TILE / PAGE_THREADS;
// The sorted tax-ID table (tax ID and dense index, 8 bytes per taxon) is searched in LDS when two workgroups still fit a CU
// beside it: a CU has 160 KiB of LDS, so a workgroup may take 80 KiB = 81920 bytes.  The widest tile (20-byte records) stages
// (5 + 1024 * 5 + 1) * 4 = 20504 bytes, the halved form's entry counts are no more (it has no table), 64 bytes go to the
// tile's own words: (81920 - 20504 - 64) / 8 = 7669 taxa; the limit is the multiple of 256 below that.
static constexpr uint32_t PAGE_LDS_TAXA = 7424;
static_assert((5 + PAGE_TILE * 5 + 1) * 4 + 64 + PAGE_LDS_TAXA * 8 <= 160 * 1024 / 2, "two workgroups of page_prepare_kernel per CU");

template <class Key, bool HALVED> struct PageRec {                  // dwords of a record; dwords staged before the tile: the one record before it
    static constexpr int DW2 = HALVED ? 3 : (sizeof(Key) == 8 ? 6 : 10);   // (twice the dwords: a halved record is one and a half)
    static constexpr int PRE = HALVED ? 2 : DW2 / 2;
    static constexpr int STAGE = PRE + PAGE_TILE * DW2 / 2 + 1;
};

// One tile of raw records -> keys, dense taxa, the low meta count (letters shared with the record before) and the marks of the
// prefix table; violations into the counter block.  The records are read once, in whole dwords, into LDS together with the one
// record before the tile; a thread then takes records t, t + 256, ... so that a wavefront's stores are consecutive.
//   table  : u32[2^tb], zero before; table[b] = number of records whose top tb key bits are <= b where a record with other top
//            bits follows (the running maximum afterwards fills the gaps): record g marks for the record BEFORE it, the last
//            record for itself.  A key with bits beyond the width marks nothing (it is counted, and the load is refused).
//   sortedIds / denseOf : the content's tax IDs ascending and their dense indices (LDSTAB: searched in LDS).
//   HALVED : records are {u32 low 30 bits, u16 dense taxon index}; the upper 30 bits are the prefix of the record's `_trie`
//            entry.  trieStart[nTrie + 1] = running sums of the entry counts (from `firstRecord` = 0), triePrefix[nTrie].  The
//            tile finds the entry of its first record with one binary search, counts the entries that begin at each of its
//            records (LDS) and takes running sums: the entry of every record.  taxOfTix[nTaxa]: the tax ID of a taxon index
//            (the order of two records with one key), denseOfTix[nTaxa]: what kasa_index_create's search gives for that ID.
template <class Key, bool HALVED, bool LDSTAB>
__global__ __launch_bounds__(PAGE_THREADS) void page_prepare_kernel(
    const uint32_t *__restrict__ raw, uint32_t n, Key *__restrict__ kmer, uint32_t *__restrict__ tax,
    typename KeyTraits<Key>::Meta *__restrict__ meta, uint32_t *__restrict__ table, int tb,
    const uint32_t *__restrict__ sortedIds, const uint32_t *__restrict__ denseOf, uint32_t nTaxa,
    const uint64_t *__restrict__ trieStart, const uint32_t *__restrict__ triePrefix, uint32_t nTrie,
    const uint32_t *__restrict__ taxOfTix, const uint32_t *__restrict__ denseOfTix, PagerCounters *__restrict__ ctr)
{
    typedef KeyTraits<Key> T;
    typedef PageRec<Key, HALVED> R;
    __shared__ uint32_t sRaw[R::STAGE];
    __shared__ uint32_t sEnt[HALVED ? PAGE_TILE : 1];               // HALVED: entries that begin at a record, then the record's entry
    __shared__ uint32_t sWave[PAGE_THREADS / 64 + 2];               // the wavefronts' totals; HALVED: the entry of the tile's first record and of the one before it
    extern __shared__ uint32_t sTab[];                              // LDSTAB: sortedIds[nTaxa], denseOf[nTaxa]
    const uint32_t t = threadIdx.x;
    const uint32_t base = blockIdx.x * (uint32_t)PAGE_TILE;
    const uint32_t cnt = min((uint32_t)PAGE_TILE, n - base);

    // the tile's dwords and the record before it, once and coalesced
    {
        const uint64_t firstDw = (uint64_t)base * R::DW2 / 2;                              // (a tile begins on a dword: 1024 * 6 bytes)
        const uint32_t nDw = (uint32_t)(((uint64_t)cnt * R::DW2 + 1) / 2);
        const uint32_t pre = base ? R::PRE : 0;
        for (uint32_t i = t; i < nDw + pre; i += PAGE_THREADS) sRaw[R::PRE - pre + i] = raw[firstDw - pre + i];
    }
    if constexpr (LDSTAB) {
        for (uint32_t i = t; i < nTaxa; i += PAGE_THREADS) { sTab[i] = sortedIds[i]; sTab[nTaxa + i] = denseOf[i]; }
    }
    if constexpr (HALVED) {
#pragma unroll
        for (int j = 0; j < PAGE_ITEMS; ++j) sEnt[t + j * PAGE_THREADS] = 0;
        if (t == 0) {                                                                      // the last entry that begins at or before the tile's first record
            uint32_t lo = 0, hi = nTrie;
            while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (trieStart[mid] <= (uint64_t)base) lo = mid; else hi = mid; }
            sWave[PAGE_THREADS / 64] = lo;
            // ... and the entry of the record before the tile: the same one, or -- when `lo` begins with the tile -- the last
            // earlier entry that has records (entries of count 0 begin where their successor does)
            uint32_t before = lo;
            if (base && trieStart[lo] == (uint64_t)base) { --before; while (before > 0 && trieStart[before] == (uint64_t)base) --before; }
            sWave[PAGE_THREADS / 64 + 1] = before;
        }
    }
    __syncthreads();
    if constexpr (HALVED) {
        const uint32_t e0 = sWave[PAGE_THREADS / 64];
        for (uint64_t e = (uint64_t)e0 + 1 + t; e < nTrie; e += PAGE_THREADS) {            // the entries the tile's records cross
            const uint64_t s = trieStart[e];
            if (s >= (uint64_t)base + cnt) break;
            atomicAdd(&sEnt[(uint32_t)(s - base)], 1u);                                    // (s > base; entries of count 0 begin where the next one does)
        }
        __syncthreads();
        // running sums over the tile's records: a thread sums four consecutive ones, the wavefronts' totals go through LDS
        uint32_t c[PAGE_ITEMS], own = 0;
#pragma unroll
        for (int j = 0; j < PAGE_ITEMS; ++j) { own += sEnt[t * PAGE_ITEMS + j]; c[j] = own; }
        const uint32_t incl = wave_incl_sum(own);
        if ((t & 63) == 63) sWave[t >> 6] = incl;
        __syncthreads();
        uint32_t before = e0 + incl - own;
        for (uint32_t w = 0; w < (t >> 6); ++w) before += sWave[w];
#pragma unroll
        for (int j = 0; j < PAGE_ITEMS; ++j) sEnt[t * PAGE_ITEMS + j] = before + c[j];
        __syncthreads();
    }

    uint32_t badOrder = 0, badTax = 0, badTix = 0;
    unsigned long long firstTix = ~0ull;
    const int shift = T::BITS - tb;
#pragma unroll 1
    for (int j = 0; j < PAGE_ITEMS; ++j) {
        const uint32_t r = t + (uint32_t)j * PAGE_THREADS;
        if (r >= cnt) break;
        const uint32_t g = base + r;
        Key key, prev = 0;
        uint32_t id, idPrev = 0, dense;
        if constexpr (HALVED) {
            // record r at byte 8 + 6 r of the staged dwords (the one before the tile at byte 2)
            auto rec = [&](uint32_t byteAt, uint32_t &low, uint32_t &tix) {
                const uint32_t w0 = sRaw[byteAt >> 2], w1 = sRaw[(byteAt >> 2) + 1];
                if (byteAt & 2u) { low = (w0 >> 16) | (w1 << 16); tix = w1 >> 16; }
                else { low = w0; tix = w1 & 0xFFFFu; }
            };
            uint32_t low, tix, lowP = 0, tixP = 0;
            rec(8u + 6u * r, low, tix);
            const uint32_t e = sEnt[r];
            key = ((uint64_t)triePrefix[e] << 30) | (low & 0x3FFFFFFFu);
            if (g) {
                rec(2u + 6u * r, lowP, tixP);
                const uint32_t eP = r ? sEnt[r - 1] : sWave[PAGE_THREADS / 64 + 1];
                prev = ((uint64_t)triePrefix[eP] << 30) | (lowP & 0x3FFFFFFFu);
            }
            if (tix >= nTaxa) { ++badTix; firstTix = min(firstTix, (unsigned long long)g); dense = 0; id = 0; }
            else { dense = denseOfTix[tix]; id = taxOfTix[tix]; }
            if (g && prev == key) idPrev = tixP < nTaxa ? taxOfTix[tixP] : 0u;
        } else {
            const uint32_t *w = sRaw + R::PRE + r * (R::DW2 / 2);
            const uint32_t *p = w - R::DW2 / 2;
            if constexpr (sizeof(Key) == 8) {
                key = (uint64_t)w[0] | ((uint64_t)w[1] << 32); id = w[2];
                if (g) { prev = (uint64_t)p[0] | ((uint64_t)p[1] << 32); idPrev = p[2]; }
            } else {
                key = ((key128)((uint64_t)w[2] | ((uint64_t)w[3] << 32)) << 64) | ((uint64_t)w[0] | ((uint64_t)w[1] << 32)); id = w[4];
                if (g) { prev = ((key128)((uint64_t)p[2] | ((uint64_t)p[3] << 32)) << 64) | ((uint64_t)p[0] | ((uint64_t)p[1] << 32)); idPrev = p[4]; }
            }
            uint32_t lo = 0, hi = nTaxa;
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                const uint32_t v = LDSTAB ? sTab[mid] : sortedIds[mid];
                if (v < id) lo = mid + 1; else hi = mid;
            }
            const bool known = lo < nTaxa && (LDSTAB ? sTab[lo] : sortedIds[lo]) == id;
            dense = known ? (LDSTAB ? sTab[nTaxa + lo] : denseOf[lo]) : 0u;
            if (!known) ++badTax;
        }
        const bool wide = (key >> T::BITS) != 0;
        // kasa_index_create's rule, record by record; it never looks at a sole record, which is looked at here
        if (g ? (prev > key || (prev == key && idPrev >= id) || wide) : (n == 1 && wide)) ++badOrder;
        kmer[g] = key;
        tax[g] = dense;
        meta[g] = g ? (typename T::Meta)lcp_letters<Key>(prev, key) : (typename T::Meta)0;
        const uint64_t b = (uint64_t)(key >> shift), bP = (uint64_t)(prev >> shift);
        if (g && bP != b && !(prev >> T::BITS)) table[bP] = g;
        if (g + 1 == n && !wide) table[b] = n;
    }
    if (badOrder) atomicAdd(&ctr->order, badOrder);
    if (badTax) atomicAdd(&ctr->unknownTax, badTax);
    if (badTix) { atomicAdd(&ctr->badTix, badTix); atomicMin(&ctr->firstBadTix, firstTix); }
}

// the `_trie` entries against the keys, from the running sums (trie_check_kernel's rule)
template <class Key>
__global__ void page_trie_check_kernel(const uint32_t *__restrict__ prefix, const uint64_t *__restrict__ start, uint32_t nTrie,
                                       const Key *__restrict__ kmer, uint32_t n, PagerCounters *__restrict__ ctr)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nTrie) return;
    const uint64_t s = start[i], e = start[i + 1];
    const int sh = 5 * (KeyTraits<Key>::LETTERS - RANGE_LETTERS);
    bool ok = e > s && e <= n;
    if (ok) ok = (uint64_t)(kmer[s] >> sh) == prefix[i] && (uint64_t)(kmer[e - 1] >> sh) == prefix[i];
    if (ok && s > 0) ok = (uint64_t)(kmer[s - 1] >> sh) < prefix[i];
    if (ok && e < n) ok = (uint64_t)(kmer[e] >> sh) > prefix[i];
    if (!ok) atomicAdd(&ctr->trie, 1u);
}

// ---- the pager --------------------------------------------------------------------------------------------------------------
struct kasa_index_pager {
    int device = 0, recordBytes = 12;
    bool wide = false;
    uint64_t maxRecords = 0, maxTrie = 0;
    uint32_t nTaxa = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    std::vector<kasa_index *> slots;
    std::vector<int64_t> held;                       // the partition a slot holds, -1: empty
    // load transients, one set: `arena` is the raw records while they are prepared, then taxSorted and order of the stable sort
    DevBuf arena, tmp, tpre, tstart, ids, dense, taxOfTix, denseOfTix, ctr;
    std::vector<uint64_t> starts;                    // host: running sums of the entry counts of the partition being loaded
    std::vector<uint32_t> taxIds;                    // host: the content's tax IDs (a refusal names one)
    uint64_t loads = 0, hits = 0, bytesCopied = 0, copyUs = 0, prepareUs = 0, refused = 0;
    size_t rec_bytes() const { return (size_t)recordBytes; }
};

static int page_table_bits(uint64_t n)
{
    int tb = 8;
    while (tb < 28 && (1ull << (tb + 1)) <= n) ++tb;
    return tb;
}

template <class Key, bool HALVED>
static int pager_dyn_lds(uint32_t nTaxa)
{
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&page_prepare_kernel<Key, HALVED, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(nTaxa * 8)));
    return KASA_OK;
}

static int pager_create_impl(int device, uint64_t maxRecords, int recordBytes, uint32_t nSlots, const uint32_t *taxIds, uint32_t nTaxa, kasa_index_pager **out)
{
    if (!out) return fail(KASA_E_ARG, "kasa_index_pager_create: out is NULL");
    *out = nullptr;
    if (recordBytes != 12 && recordBytes != 20 && recordBytes != 6)
        return fail(KASA_E_ARG, "kasa_index_pager_create: records are 12 bytes {u64 kmer, u32 taxid}, 20 bytes {u64 low, u64 high, u32 taxid} (k <= 25) or 6 bytes (halved), got %d", recordBytes);
    if (nSlots < 1 || nSlots > 64) return fail(KASA_E_ARG, "kasa_index_pager_create: %u slots (1 to 64)", nSlots);
    if (maxRecords == 0) return fail(KASA_E_ARG, "kasa_index_pager_create: maxRecords is 0");
    if (maxRecords >= 0xFFFFFFF0ull) return fail(KASA_E_LIMIT, "kasa_index_pager_create: %llu records exceed the 32-bit position range of this build", (unsigned long long)maxRecords);
    if (!taxIds || nTaxa < 2) return fail(KASA_E_ARG, "kasa_index_pager_create: content mapping missing");
    if (nTaxa >= (1u << 22)) return fail(KASA_E_LIMIT, "kasa_index_pager_create: %u taxa exceed the 2^22 taxon indices an event record can name", nTaxa);
    int ndev = 0;
    kasa_device_count(&ndev);
    if (device < 0 || device >= ndev) return fail(KASA_E_HIP, "kasa_index_pager_create: no HIP device %d (found %d)", device, ndev);
    HIPCHK(hipSetDevice(device));
    (void)hipGetLastError();
    kasa_index_pager *pg = new kasa_index_pager();
    pg->device = device; pg->recordBytes = recordBytes; pg->wide = recordBytes == 20; pg->maxRecords = maxRecords; pg->nTaxa = nTaxa;
    pg->maxTrie = std::min<uint64_t>(maxRecords, 1ull << (5 * RANGE_LETTERS));   // an entry has at least one record, a prefix 30 bits
    pg->taxIds.assign(taxIds, taxIds + nTaxa);
    pg->starts.reserve(pg->maxTrie + 1);
    auto bail = [&](int code) { kasa_index_pager_destroy(pg); return code; };
#define TRY(x) do { const int rc_ = (x); if (rc_ != KASA_OK) return bail(rc_); } while (0)
#define TRYHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return bail(fail(e_ == hipErrorOutOfMemory ? KASA_E_NOMEM : KASA_E_HIP, "%s failed: %s", #x, hipGetErrorString(e_))); } while (0)
    TRYHIP(hipStreamCreateWithFlags(&pg->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : pg->ev) TRYHIP(hipEventCreate(&e));
    const size_t keyBytes = pg->wide ? 16 : 8, metaBytes = pg->wide ? 2 : 1;
    const uint64_t maxTable = 1ull << page_table_bits(maxRecords);
    for (uint32_t s = 0; s < nSlots; ++s) {
        kasa_index *ix = new kasa_index();
        pg->slots.push_back(ix); pg->held.push_back(-1);
        ix->device = device; ix->n = 0; ix->nTaxa = nTaxa; ix->wide = pg->wide;
        ix->bound = std::make_shared<std::atomic<int>>(0);
        TRY(ix->kmer.reserve(maxRecords * keyBytes)); TRY(ix->tax.reserve(maxRecords * 4)); TRY(ix->meta.reserve(maxRecords * metaBytes));
        TRY(ix->table.reserve(maxTable * 4));
    }
    TRY(pg->arena.reserve(std::max<uint64_t>(maxRecords * pg->rec_bytes() + 8, maxRecords * 8)));
    TRY(pg->tpre.reserve((pg->maxTrie + 1) * 4)); TRY(pg->tstart.reserve((pg->maxTrie + 1) * 8));
    TRY(pg->ctr.reserve(PAGER_COUNTER_BYTES));
    // the rocPRIM scratch of the largest load: the stable sort by taxon and the table's running maximum
    {
        unsigned bits = 1;
        while ((1ull << bits) < nTaxa) ++bits;
        size_t sortBytes = 0, scanBytes = 0;
        rocprim::counting_iterator<uint32_t> cnt(0);
        uint32_t *none = nullptr;
        TRYHIP(rocprim::radix_sort_pairs(nullptr, sortBytes, none, none, cnt, none, (size_t)maxRecords, 0u, bits, pg->stream));
        TRYHIP(rocprim::inclusive_scan(nullptr, scanBytes, none, none, (size_t)maxTable, rocprim::maximum<uint32_t>(), pg->stream));
        TRY(pg->tmp.reserve(std::max(sortBytes, scanBytes)));
    }
    // taxid -> dense index (Compare.hpp:139-143), as kasa_index_create makes it; for the halved form per taxon index
    {
        std::vector<uint32_t> perm(nTaxa), sid(nTaxa), did(nTaxa), ofTix(nTaxa);
        for (uint32_t i = 0; i < nTaxa; ++i) perm[i] = i;
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return taxIds[a] < taxIds[b]; });
        for (uint32_t i = 0; i < nTaxa; ++i) { sid[i] = taxIds[perm[i]]; did[i] = perm[i]; }
        for (uint32_t i = 0; i < nTaxa; ++i) ofTix[i] = did[std::lower_bound(sid.begin(), sid.end(), taxIds[i]) - sid.begin()];
        TRY(pg->ids.reserve(nTaxa * 4)); TRY(pg->dense.reserve(nTaxa * 4)); TRY(pg->taxOfTix.reserve(nTaxa * 4)); TRY(pg->denseOfTix.reserve(nTaxa * 4));
        TRYHIP(hipMemcpyAsync(pg->ids.p, sid.data(), nTaxa * 4, hipMemcpyHostToDevice, pg->stream));
        TRYHIP(hipMemcpyAsync(pg->dense.p, did.data(), nTaxa * 4, hipMemcpyHostToDevice, pg->stream));
        TRYHIP(hipMemcpyAsync(pg->taxOfTix.p, taxIds, nTaxa * 4, hipMemcpyHostToDevice, pg->stream));
        TRYHIP(hipMemcpyAsync(pg->denseOfTix.p, ofTix.data(), nTaxa * 4, hipMemcpyHostToDevice, pg->stream));
        TRYHIP(hipStreamSynchronize(pg->stream));
    }
    if (nTaxa <= PAGE_LDS_TAXA && recordBytes != 6) TRY(pg->wide ? (pager_dyn_lds<key128, false>(nTaxa)) : (pager_dyn_lds<uint64_t, false>(nTaxa)));
#undef TRY
#undef TRYHIP
    *out = pg;
    return KASA_OK;
}

extern "C" int kasa_index_pager_create(int device, uint64_t maxRecords, int recordBytes, uint32_t nSlots, const uint32_t *taxIds, uint32_t nTaxa, kasa_index_pager **out)
{
    KASA_GUARDED(pager_create_impl(device, maxRecords, recordBytes, nSlots, taxIds, nTaxa, out))
}

extern "C" int kasa_index_pager_destroy(kasa_index_pager *pg)
{
    if (!pg) return KASA_OK;
    (void)hipSetDevice(pg->device);
    if (pg->stream) (void)hipStreamSynchronize(pg->stream);
    for (kasa_index *ix : pg->slots) { ix->kmer.release(); ix->tax.release(); ix->meta.release(); ix->table.release(); delete ix; }
    for (hipEvent_t e : pg->ev) if (e) (void)hipEventDestroy(e);
    if (pg->stream) (void)hipStreamDestroy(pg->stream);
    delete pg;                                       // (the transients go with it)
    return KASA_OK;
}

template <class Key, bool HALVED>
static int pager_load_impl(kasa_index_pager *pg, kasa_index *ix, const void *records, uint64_t nRecords,
                           const uint32_t *triePrefix, const uint64_t *trieCount, uint64_t nTrie)
{
    typedef KeyTraits<Key> T;
    typedef typename T::Meta Meta;
    const uint32_t n = (uint32_t)nRecords;
    const size_t REC = pg->rec_bytes();
    const bool haveTrie = triePrefix && trieCount && nTrie;
    hipStream_t st = pg->stream;
    if (haveTrie) {
        if (nTrie > pg->maxTrie) return fail(KASA_E_LIMIT, "kasa_index_pager_load: %llu trie entries, the pager was made for %llu", (unsigned long long)nTrie, (unsigned long long)pg->maxTrie);
        pg->starts.resize(nTrie + 1);
        uint64_t run = 0;
        for (uint64_t i = 0; i < nTrie; ++i) { pg->starts[i] = run; run += trieCount[i]; }
        pg->starts[nTrie] = run;
        if (HALVED && run > nRecords) return fail(KASA_E_ARG, "kasa_index_create: the trie file counts more entries than the index has");
        if (run != nRecords) return fail(KASA_E_ARG, "kasa_index_create: the trie file counts %llu entries, the index has %llu", (unsigned long long)run, (unsigned long long)nRecords);
    }
    // every return below leaves the stream idle
    auto done = [&](int code) { (void)hipStreamSynchronize(st); return code; };
#define TRY(x) do { const int rc_ = (x); if (rc_ != KASA_OK) return done(rc_); } while (0)
#define TRYHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return done(fail(e_ == hipErrorOutOfMemory ? KASA_E_NOMEM : KASA_E_HIP, "%s failed: %s", #x, hipGetErrorString(e_))); } while (0)
    const int tb = page_table_bits(n);
    const uint64_t nb = 1ull << tb;
    PagerCounters *ctr = pg->ctr.as<PagerCounters>();
    TRYHIP(hipEventRecord(pg->ev[0], st));
    TRYHIP(hipMemcpyAsync(pg->arena.p, records, (size_t)n * REC, hipMemcpyDefault, st));   // host memory of any kind (the mapped file) or device memory
    if (haveTrie) {
        TRYHIP(hipMemcpyAsync(pg->tpre.p, triePrefix, nTrie * 4, hipMemcpyHostToDevice, st));
        TRYHIP(hipMemcpyAsync(pg->tstart.p, pg->starts.data(), (nTrie + 1) * 8, hipMemcpyHostToDevice, st));
    }
    TRYHIP(hipEventRecord(pg->ev[1], st));
    TRYHIP(hipMemsetAsync(ctr, 0, PAGER_COUNTER_BYTES, st));
    TRYHIP(hipMemsetAsync(&ctr->firstBadTix, 0xFF, sizeof(ctr->firstBadTix), st));
    TRYHIP(hipMemsetAsync(ix->table.p, 0, nb * 4, st));
    const unsigned tiles = blocks_for(n, PAGE_TILE);
    const bool lds = !HALVED && pg->nTaxa <= PAGE_LDS_TAXA;
    if (lds)
        page_prepare_kernel<Key, HALVED, true><<<tiles, PAGE_THREADS, (size_t)pg->nTaxa * 8, st>>>(pg->arena.as<uint32_t>(), n, ix->kmer.as<Key>(), ix->tax.as<uint32_t>(), ix->meta.as<Meta>(),
            ix->table.as<uint32_t>(), tb, pg->ids.as<uint32_t>(), pg->dense.as<uint32_t>(), pg->nTaxa, pg->tstart.as<uint64_t>(), pg->tpre.as<uint32_t>(), (uint32_t)nTrie,
            pg->taxOfTix.as<uint32_t>(), pg->denseOfTix.as<uint32_t>(), ctr);
    else
        page_prepare_kernel<Key, HALVED, false><<<tiles, PAGE_THREADS, 0, st>>>(pg->arena.as<uint32_t>(), n, ix->kmer.as<Key>(), ix->tax.as<uint32_t>(), ix->meta.as<Meta>(),
            ix->table.as<uint32_t>(), tb, pg->ids.as<uint32_t>(), pg->dense.as<uint32_t>(), pg->nTaxa, pg->tstart.as<uint64_t>(), pg->tpre.as<uint32_t>(), (uint32_t)nTrie,
            pg->taxOfTix.as<uint32_t>(), pg->denseOfTix.as<uint32_t>(), ctr);
    TRYHIP(hipGetLastError());
    PagerCounters h;
    TRY(fetch(st, h, ctr));
    if (h.badTix) {
        uint16_t tix = 0;
        memcpy(&tix, static_cast<const uint8_t *>(records) + h.firstBadTix * 6 + 4, 2);
        return done(fail(KASA_E_ARG, "kasa_index_create: halved index entry %llu names taxon index %u of %u", h.firstBadTix, (unsigned)tix, pg->nTaxa));
    }
    if (h.order) return done(fail(KASA_E_ARG, "kasa_index_create: the index is not sorted by (kmer, taxid), not unique, or uses more than %d key bits (%u violations)", T::BITS, h.order));
    if (h.unknownTax) return done(fail(KASA_E_ARG, "kasa_index_create: %u index entries carry a tax ID the content file does not know", h.unknownTax));
    // meta's upper count: letters shared with the nearest earlier entry of the same taxon (the raw records are done with: their
    // place is the sort's)
    {
        uint32_t *taxSorted = pg->arena.as<uint32_t>(), *order = taxSorted + pg->maxRecords;
        unsigned bits = 1;
        while ((1ull << bits) < pg->nTaxa) ++bits;
        rocprim::counting_iterator<uint32_t> cnt(0);
        TRY(dev_sort_pairs(pg->tmp, st, ix->tax.as<uint32_t>(), taxSorted, cnt, order, (size_t)n, 0u, bits));
        dup_level_kernel<Key><<<blocks_for(n, 256), 256, 0, st>>>(taxSorted, order, ix->kmer.as<Key>(), n, ix->meta.as<Meta>());
    }
    TRY(dev_inclusive_scan(pg->tmp, st, ix->table.as<uint32_t>(), ix->table.as<uint32_t>(), (size_t)nb, rocprim::maximum<uint32_t>()));
    if (haveTrie) page_trie_check_kernel<Key><<<blocks_for(nTrie, 256), 256, 0, st>>>(pg->tpre.as<uint32_t>(), pg->tstart.as<uint64_t>(), (uint32_t)nTrie, ix->kmer.as<Key>(), n, ctr);
    TRYHIP(hipGetLastError());
    TRYHIP(hipEventRecord(pg->ev[2], st));
    TRY(fetch(st, h, ctr));
    if (h.trie) return done(fail(KASA_E_ARG, "kasa_index_create: the trie file does not match the index (%u ranges differ)", h.trie));
    float copyMs = 0.0f, prepMs = 0.0f;
    TRYHIP(hipEventElapsedTime(&copyMs, pg->ev[0], pg->ev[1]));
    TRYHIP(hipEventElapsedTime(&prepMs, pg->ev[1], pg->ev[2]));
#undef TRY
#undef TRYHIP
    pg->copyUs += (uint64_t)(copyMs * 1000.0f); pg->prepareUs += (uint64_t)(prepMs * 1000.0f);
    pg->bytesCopied += (uint64_t)n * REC + (haveTrie ? nTrie * 12 + 8 : 0);
    ix->n = n; ix->tb = tb;
    return KASA_OK;
}

extern "C" int kasa_index_pager_load(kasa_index_pager *pg, uint32_t slot, uint64_t partitionId, const void *records, uint64_t nRecords,
                                     const uint32_t *triePrefix, const uint64_t *trieCount, uint64_t nTrie)
{
    if (!pg) return fail(KASA_E_ARG, "kasa_index_pager_load: pager is NULL");
    if (slot >= pg->slots.size()) return fail(KASA_E_ARG, "kasa_index_pager_load: slot %u of %zu", slot, pg->slots.size());
    if (partitionId >> 63) return fail(KASA_E_ARG, "kasa_index_pager_load: partition ids are below 2^63");
    kasa_index *ix = pg->slots[slot];
    if (pg->held[slot] == (int64_t)partitionId) { pg->hits++; return KASA_OK; }
    if (ix->bound->load() > 0) return fail(KASA_E_STATE, "kasa_index_pager_load: %d context(s) are bound to slot %u (kasa_ctx_set_index to another index, or destroy them, first)", ix->bound->load(), slot);
    pg->held[slot] = -1; ix->n = 0;                  // empty until the load has gone through
    pg->refused++;                                   // (taken back below)
    if (!records && nRecords) return fail(KASA_E_ARG, "kasa_index_create: records is NULL");
    if (nRecords == 0) return fail(KASA_E_ARG, "The index file cannot be found or is empty!");
    if (nRecords > pg->maxRecords) return fail(KASA_E_LIMIT, "kasa_index_pager_load: %llu records, the pager's slots hold %llu", (unsigned long long)nRecords, (unsigned long long)pg->maxRecords);
    if (pg->recordBytes == 6 && (!triePrefix || !trieCount || !nTrie)) return fail(KASA_E_ARG, "kasa_index_create: a halved index needs its trie and content mapping");
    HIPCHK(hipSetDevice(pg->device));
    int rc;
    try {
        rc = pg->recordBytes == 20 ? pager_load_impl<key128, false>(pg, ix, records, nRecords, triePrefix, trieCount, nTrie)
           : pg->recordBytes == 6 ? pager_load_impl<uint64_t, true>(pg, ix, records, nRecords, triePrefix, trieCount, nTrie)
                                  : pager_load_impl<uint64_t, false>(pg, ix, records, nRecords, triePrefix, trieCount, nTrie);
    } catch (const std::bad_alloc &) { rc = fail(KASA_E_NOMEM, "host allocation failed"); }
    if (rc) return rc;
    pg->refused--; pg->loads++;
    pg->held[slot] = (int64_t)partitionId;
    return KASA_OK;
}

extern "C" int kasa_index_pager_index(kasa_index_pager *pg, uint32_t slot, const kasa_index **ix)
{
    if (!pg || !ix) return fail(KASA_E_ARG, "kasa_index_pager_index: NULL argument");
    *ix = nullptr;
    if (slot >= pg->slots.size()) return fail(KASA_E_ARG, "kasa_index_pager_index: slot %u of %zu", slot, pg->slots.size());
    if (pg->held[slot] < 0) return fail(KASA_E_STATE, "kasa_index_pager_index: slot %u is empty", slot);
    *ix = pg->slots[slot];
    return KASA_OK;
}

extern "C" int kasa_index_pager_stats(kasa_index_pager *pg, uint64_t out[8])
{
    if (!pg || !out) return fail(KASA_E_ARG, "kasa_index_pager_stats: NULL argument");
    out[0] = pg->loads; out[1] = pg->hits; out[2] = pg->bytesCopied; out[3] = pg->copyUs; out[4] = pg->prepareUs; out[5] = pg->refused;
    uint64_t dev = pg->arena.cap + pg->tmp.cap + pg->tpre.cap + pg->tstart.cap + pg->ids.cap + pg->dense.cap + pg->taxOfTix.cap + pg->denseOfTix.cap + pg->ctr.cap;
    for (const kasa_index *ix : pg->slots) dev += ix->bytes();
    out[6] = dev; out[7] = pg->nTaxa <= PAGE_LDS_TAXA && pg->recordBytes != 6 ? 1 : 0;
    return KASA_OK;
}

extern "C" int kasa_index_pager_tile(uint32_t *tileRecords, uint32_t *ldsTaxa)
{
    if (tileRecords) *tileRecords = PAGE_TILE;
    if (ldsTaxa) *ldsTaxa = PAGE_LDS_TAXA;
    return KASA_OK;
}

// ---- a context moves to another index ----------------------------------------------------------------------------------------
extern "C" int kasa_ctx_set_index(kasa_ctx *c, const kasa_index *ix)
{
    if (!c || !ix) return fail(KASA_E_ARG, "kasa_ctx_set_index: NULL argument");
    if (ix->device != c->ix->device) return fail(KASA_E_ARG, "kasa_ctx_set_index: the index lies on device %d, the context works on device %d", ix->device, c->ix->device);
    if (ix->wide != c->ix->wide) return fail(KASA_E_ARG, "kasa_ctx_set_index: the index has %d-letter keys, the context was made for %d", ix->letters(), c->ix->letters());
    if (ix->nTaxa != c->ix->nTaxa) return fail(KASA_E_ARG, "kasa_ctx_set_index: the index names %u taxa, the context's tables hold %u", ix->nTaxa, c->ix->nTaxa);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));        // nothing of the context still reads the index it leaves
    if (ix->bound) ++*ix->bound;
    if (c->bound) --*c->bound;
    c->bound = ix->bound;
    c->ix = ix;
    c->state = 0;                                    // an uploaded batch was looked up in the other index
    coh_forget(c);
    return KASA_OK;
}

// ---- a slice's pool gets a home with the owner -------------------------------------------------------------------------------
extern "C" int kasa_batch_pool_keep(kasa_ctx *c, const uint32_t *poolDev, uint64_t nPoolWords, const uint32_t **keptDev)
{
    if (!c || !keptDev || (nPoolWords && !poolDev)) return fail(KASA_E_ARG, "kasa_batch_pool_keep: NULL argument");
    *keptDev = nullptr;
    if (c->state < 3) return fail(KASA_E_STATE, "kasa_batch_pool_keep: batch not sorted");
    HIPCHK(hipSetDevice(c->device));
    try { if (c->keptUsed == c->kept.size()) c->kept.emplace_back(); }
    catch (const std::bad_alloc &) { return fail(KASA_E_NOMEM, "host allocation failed"); }
    DevBuf &b = c->kept[c->keptUsed];
    if (int rc = b.reserve(std::max<uint64_t>(nPoolWords, 1) * 4)) return rc;
    if (nPoolWords) HIPCHK(hipMemcpyAsync(b.p, poolDev, nPoolWords * 4, hipMemcpyDefault, c->stream));   // this device's memory or another's
    HIPCHK(hipStreamSynchronize(c->stream));
    c->keptUsed++;
    *keptDev = b.as<uint32_t>();
    return KASA_OK;
}

// ---- test tap: the arrays of an index ------------------------------------------------------------------------------------------
extern "C" int kasa_index_fetch(const kasa_index *ix, int what, void *out, uint64_t bytes)
{
    if (!ix || !out) return fail(KASA_E_ARG, "kasa_index_fetch: NULL argument");
    const void *src = nullptr;
    uint64_t want = 0;
    switch (what) {
    case KASA_INDEX_KEYS: src = ix->kmer.p; want = ix->n * (ix->wide ? 16 : 8); break;
    case KASA_INDEX_TAXA: src = ix->tax.p; want = ix->n * 4; break;
    case KASA_INDEX_META: src = ix->meta.p; want = ix->n * (ix->wide ? 2 : 1); break;
    case KASA_INDEX_TABLE: src = ix->table.p; want = (1ull << ix->tb) * 4; break;
    case KASA_INDEX_TABLE_BITS: want = 4; break;
    default: return fail(KASA_E_ARG, "kasa_index_fetch: what = %d", what);
    }
    if (bytes != want) return fail(KASA_E_ARG, "kasa_index_fetch: %llu bytes asked for, this array has %llu", (unsigned long long)bytes, (unsigned long long)want);
    if (what == KASA_INDEX_TABLE_BITS) { const int32_t tb = ix->tb; memcpy(out, &tb, 4); return KASA_OK; }
    HIPCHK(hipSetDevice(ix->device));
    if (want) HIPCHK(hipMemcpy(out, src, want, hipMemcpyDeviceToHost));
    return KASA_OK;
}
