// kasa_spill.h -- `kASA build` of an index larger than device memory, behind kasa_build_set_resident / finish_begin / slab /
// fetch_slab / finish_end / spill_stats of include/kasa_hip.h.  Included after kasa_build.h and kasa_edit.h.
//
// Reference: any size through STXXL temporaries (Build.hpp:305-477).  Here the runs of the bricks (kasa_build.h) leave the device
// for pageable host memory once they outgrow the resident budget, and the finish walks the key space in slabs:
//   spill   : a run's (key, rank) arrays copied down and released; once a builder spills, every new run follows right after
//             unique_into.  The copies are hipMemcpyAsync on the builder's stream from and to pageable memory: the runtime
//             stages them through its own page-locked buffers, the runs themselves are never page-locked.
//   plan    : kasa_spill_plan.h (host only): slabs as intervals of 6-letter prefixes, greedy under the budget, per run a slice
//   slab    : the slices uploaded and merged pairwise (merge_runs), then finish_slab of kasa_build.h: bld_emit_kernel and the
//             bld_trie_* kernels on the slab's result; bld_freq_kernel adds to histograms that live from the first slab to the
//             last, bld_freq_final_kernel runs once.  No kernel of its own.
// The finish has one body for every builder: runs that stayed on the device are one slab, which finish_begin_impl merges, edits
// (kasa_edit.h) and hands to the same finish_slab; kasa_build_slab(b, 0) then only reports it.
// A cut between two prefixes splits no k-mer, no duplicate pair and no trie entry ({count, prefix}, no global offsets), and the
// frequency rows are sums over records: the slabs' records and trie entries concatenate to what the in-core finish gives.
//
// Device bytes per input record of a slab, at their peak: the last merge holds two generations of
// (key, rank) and one count per MERGE_ITEMS outputs, 2 (keyBytes + 4) + 1; the emit holds the merged run, the file records, a
// flag word and a scan slot, (keyBytes + 4) + (keyBytes + 4) + 4 + 8 = 36 (64-bit keys) or 52 (128-bit).  The trie's 20 bytes
// per distinct prefix (at most 2^30 of them) come out of the head-room.
#pragma once

namespace kasa_build_impl {

static inline uint64_t spill_bytes_per_record(const kasa_builder *b) { return 2 * ((uint64_t)b->keyBytes() + 4) + 12; }
static constexpr double SPILL_HEADROOM = 0.8;          // the share of the free device memory a slab is planned into

struct SpillTimer {
    double *acc;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit SpillTimer(double *a) : acc(a) {}
    ~SpillTimer() { *acc += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
};

// one run: device -> pageable host memory, the device arrays released
template <class Key>
static int spill_run(kasa_builder *b, kasa_builder::Run &r)
{
    if (r.n) {
        kasa_spill_plan::HostRun h;
        h.k = malloc((size_t)r.n * sizeof(Key));
        h.v = static_cast<uint32_t *>(malloc((size_t)r.n * 4));
        if (!h.k || !h.v) return fail(KASA_E_NOMEM, "kasa_build: host allocation of %llu bytes for a spilled run failed", (unsigned long long)(r.n * (sizeof(Key) + 4)));
        h.n = r.n;
        {
            SpillTimer t(&b->usDown);
            HIPCHK(hipMemcpyAsync(h.k, r.k.p, (size_t)r.n * sizeof(Key), hipMemcpyDeviceToHost, b->stream));
            HIPCHK(hipMemcpyAsync(h.v, r.v.p, (size_t)r.n * 4, hipMemcpyDeviceToHost, b->stream));
            HIPCHK(hipStreamSynchronize(b->stream));
        }
        b->hostRuns.push_back(std::move(h));
        ++b->spillRuns; b->spillRecords += r.n;
    }
    r.k.release(); r.v.release(); r.n = 0;
    return KASA_OK;
}

template <class Key>
static int spill_all_runs(kasa_builder *b)
{
    int rc;
    b->spilled = true;
    for (kasa_builder::Run &r : b->runs) if ((rc = spill_run<Key>(b, r))) return rc;
    b->runs.clear();
    return KASA_OK;
}

// after a brick's run joined b->runs: does the builder spill (now, or since an earlier brick)?
template <class Key>
static int spill_after_brick(kasa_builder *b)
{
    if (b->edited) return KASA_OK;                                     // edits need the runs on the device
    if (!b->spilled) {
        uint64_t held = 0;
        for (const kasa_builder::Run &r : b->runs) held += r.n;
        if (b->resident) { if (held <= b->resident) return KASA_OK; }
        else {
            // automatic: the in-core finish of what is held fits for sure while its peak stays inside the head-room of the memory
            // that is free beside the brick buffers (the runs' own bytes are part of that peak)
            size_t freeB = 0, totalB = 0;
            HIPCHK(hipMemGetInfo(&freeB, &totalB));
            const double avail = SPILL_HEADROOM * ((double)freeB + (double)held * ((double)b->keyBytes() + 4));
            if ((double)held * (double)spill_bytes_per_record(b) <= avail) return KASA_OK;
        }
    }
    return spill_all_runs<Key>(b);
}

// kasa_build_finish_begin.  Runs on the device: merged, edited and emitted here, as the one slab kasa_build_slab(b, 0) reports.
// Runs in host memory: the plan of the slabs, which kasa_build_slab brings up one by one.
template <class Key>
static int finish_begin_impl(kasa_builder *b, uint64_t *nSlabs)
{
    int rc;
    if ((rc = flush_brick<Key>(b))) return rc;
    // the brick buffers are not needed any more: their memory goes to the merges
    for (DevBuf *d : {&b->dBases, &b->dBaseOff, &b->dSeqOff, &b->dSeqRank, &b->dLong, &b->kA, &b->vA, &b->kB, &b->vB, &b->sortTmp, &b->flags}) d->release();
    b->totalRec = 0; b->totalTrie = 0;
    if (!b->spilled) {
        {
            StageClock clk(&b->ms[2], b->stream);
            rc = merge_runs<Key>(b, b->runs);
            clk.stop();
        }
        // merge_two's memory check refused: the runs are whole (merge_runs), the build goes on by slabs -- edits need them on the device
        if (rc == KASA_E_LIMIT && !b->edited) rc = spill_all_runs<Key>(b);
        if (rc) return rc;
    }
    if (!b->spilled) {
        if (b->runs.empty()) b->runs.emplace_back();
        b->result = std::move(b->runs[0]);
        b->runs.clear();
        if ((rc = edit_finish<Key>(b))) return rc;                   // nothing when no kasa_build_add_index/drop_taxa/shrink was called
        if ((rc = finish_slab<Key>(b, true, true))) return rc;
    } else {
        uint64_t budget = b->resident;
        if (!budget) {
            size_t freeB = 0, totalB = 0;
            HIPCHK(hipMemGetInfo(&freeB, &totalB));
            budget = std::max<uint64_t>(1, (uint64_t)(SPILL_HEADROOM * (double)freeB) / spill_bytes_per_record(b));
        }
        std::vector<const Key *> keys;
        std::vector<uint64_t> n;
        for (const kasa_spill_plan::HostRun &h : b->hostRuns) { keys.push_back(static_cast<const Key *>(h.k)); n.push_back(h.n); }
        if (!kasa_spill_plan::make_plan<Key>(keys.data(), n.data(), keys.size(), KeyTraits<Key>::LETTERS, budget, b->plan))
            return fail(KASA_E_LIMIT, "kasa_build_finish: %s (a slab holds whole 6-letter prefixes)", kasa_spill_plan::refusal_text(b->plan).c_str());
        b->result.n = 0; b->nTrie = 0;
    }
    b->state = kasa_builder::SLABS; b->slabNext = 0;
    b->records = b->spilled ? kasa_builder::BY_SLAB : kasa_builder::ON_DEVICE;
    if (nSlabs) *nSlabs = b->nSlabs();
    return KASA_OK;
}

// slab `s` of a spilled builder: slices up, merged, emitted; its records and trie stay on the device until the next slab
template <class Key>
static int slab_impl(kasa_builder *b, uint64_t s)
{
    int rc;
    const kasa_spill_plan::Slab &sl = b->plan.slabs[(size_t)s];
    const bool last = s + 1 == b->plan.slabs.size();
    for (DevBuf *d : {&b->rec, &b->trieFirst, &b->triePrefix, &b->trieCount}) d->release();   // (the slab before)
    std::vector<kasa_builder::Run> runs;
    {
        SpillTimer t(&b->usUp);
        for (size_t r = 0; r < b->hostRuns.size(); ++r) {
            const uint64_t lo = sl.lo[r], n = sl.hi[r] - lo;
            if (!n) continue;
            kasa_builder::Run d;
            if ((rc = d.k.reserve(n * sizeof(Key) + 64)) || (rc = d.v.reserve(n * 4 + 64))) return rc;
            HIPCHK(hipMemcpyAsync(d.k.p, static_cast<const Key *>(b->hostRuns[r].k) + lo, (size_t)n * sizeof(Key), hipMemcpyHostToDevice, b->stream));
            HIPCHK(hipMemcpyAsync(d.v.p, b->hostRuns[r].v + lo, (size_t)n * 4, hipMemcpyHostToDevice, b->stream));
            d.n = n;
            runs.push_back(std::move(d));
        }
        HIPCHK(hipStreamSynchronize(b->stream));
    }
    {
        StageClock clk(&b->ms[2], b->stream);
        if ((rc = merge_runs<Key>(b, runs))) return rc;
        clk.stop();
    }
    if (runs.empty()) runs.emplace_back();
    b->result = std::move(runs[0]);
    if ((rc = finish_slab<Key>(b, s == 0, last))) return rc;
    if (last) b->hostRuns.clear();                                     // the host memory of the runs goes back
    return KASA_OK;
}

static int build_slab_impl(kasa_builder *b, uint64_t slab, uint64_t *nRecords, uint64_t *nTrie)
{
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->state != kasa_builder::SLABS) return fail(KASA_E_STATE, b->state == kasa_builder::ADDING ? "kasa_build_slab: kasa_build_finish_begin first" : "kasa_build_slab: the build is finished");
    if (slab != b->slabNext || slab >= b->nSlabs())
        return fail(KASA_E_STATE, "kasa_build_slab: slab %llu asked, slab %llu of %llu is next (the slabs are taken in order, each once)", (unsigned long long)slab,
                    (unsigned long long)b->slabNext, (unsigned long long)b->nSlabs());
    HIPCHK(hipSetDevice(b->device));
    if (b->spilled) { if (int rc = b->wide ? slab_impl<key128>(b, slab) : slab_impl<uint64_t>(b, slab)) return rc; }   // (else: finish_begin made the one slab)
    ++b->slabNext;
    if (nRecords) *nRecords = b->result.n;
    if (nTrie) *nTrie = b->nTrie;
    return KASA_OK;
}

static int build_fetch_slab_impl(kasa_builder *b, uint64_t first, uint64_t count, void *records, uint32_t *triePrefix, uint64_t *trieCount)
{
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->state != kasa_builder::SLABS || b->slabNext == 0) return fail(KASA_E_STATE, "kasa_build_fetch_slab: no slab is current (kasa_build_slab first, kasa_build_finish_end after the last fetch)");
    if (first > b->result.n || count > b->result.n - first)
        return fail(KASA_E_ARG, "kasa_build_fetch_slab: [%llu, +%llu) outside the slab's %llu records", (unsigned long long)first, (unsigned long long)count, (unsigned long long)b->result.n);
    HIPCHK(hipSetDevice(b->device));
    SpillTimer t(&b->usDown);
    const uint64_t rb = (uint64_t)b->recBytes();
    if (records && count) HIPCHK(hipMemcpyAsync(records, b->rec.as<uint8_t>() + first * rb, count * rb, hipMemcpyDeviceToHost, b->stream));
    if (triePrefix && b->nTrie) HIPCHK(hipMemcpyAsync(triePrefix, b->triePrefix.p, b->nTrie * 4, hipMemcpyDeviceToHost, b->stream));
    if (trieCount && b->nTrie) HIPCHK(hipMemcpyAsync(trieCount, b->trieCount.p, b->nTrie * 8, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return KASA_OK;
}

static int build_finish_end_impl(kasa_builder *b, uint64_t *nRecords, uint64_t *nTrie)
{
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->state != kasa_builder::SLABS) return fail(KASA_E_STATE, b->state == kasa_builder::ADDING ? "kasa_build_finish_end: kasa_build_finish_begin first" : "kasa_build_finish_end: called twice");
    if (b->slabNext != b->nSlabs())
        return fail(KASA_E_STATE, "kasa_build_finish_end: %llu of %llu slabs were taken", (unsigned long long)b->slabNext, (unsigned long long)b->nSlabs());
    if (b->records != kasa_builder::ON_DEVICE)                         // (the last slab; records on the device stay for kasa_build_fetch)
        for (DevBuf *d : {&b->rec, &b->trieFirst, &b->triePrefix, &b->trieCount}) d->release();
    b->result.n = b->totalRec; b->nTrie = b->totalTrie;
    b->state = kasa_builder::DONE;
    if (nRecords) *nRecords = b->result.n;
    if (nTrie) *nTrie = b->nTrie;
    return KASA_OK;
}

// kasa_build_finish: every slab in one call; a spilled builder's records and trie entries are gathered in host memory
template <class Key>
static int finish_all(kasa_builder *b, uint64_t *nRecords, uint64_t *nTrie)
{
    int rc;
    uint64_t nSlabs = 0;
    if ((rc = finish_begin_impl<Key>(b, &nSlabs))) return rc;
    for (uint64_t s = 0; s < nSlabs; ++s) {
        uint64_t n = 0, m = 0;
        if ((rc = build_slab_impl(b, s, &n, &m))) return rc;
        if (b->records == kasa_builder::ON_DEVICE) continue;
        const size_t rb = (size_t)b->recBytes(), at = b->hRec.size(), tAt = b->hTriePrefix.size();
        b->hRec.resize(at + (size_t)n * rb);
        b->hTriePrefix.resize(tAt + (size_t)m);
        b->hTrieCount.resize(tAt + (size_t)m);
        if ((rc = build_fetch_slab_impl(b, 0, n, b->hRec.data() + at, b->hTriePrefix.data() + tAt, b->hTrieCount.data() + tAt))) return rc;
    }
    if ((rc = build_finish_end_impl(b, nRecords, nTrie))) return rc;
    if (b->records == kasa_builder::BY_SLAB) b->records = kasa_builder::GATHERED;
    return KASA_OK;
}

} // namespace kasa_build_impl

extern "C" int kasa_build_set_resident(kasa_builder *b, uint64_t maxResidentRecords)
{
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->added || b->state != kasa_builder::ADDING) return fail(KASA_E_STATE, "kasa_build_set_resident: the budget is set before the first kasa_build_add");
    if (b->edited) return fail(KASA_E_STATE, "kasa_build_set_resident: edits need the runs on the device");
    b->resident = maxResidentRecords;
    return KASA_OK;
}

extern "C" int kasa_build_finish_begin(kasa_builder *b, uint64_t *nSlabs)
{
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->state != kasa_builder::ADDING) return fail(KASA_E_STATE, "kasa_build_finish_begin: called twice");
    HIPCHK(hipSetDevice(b->device));
    KASA_GUARDED(b->wide ? kasa_build_impl::finish_begin_impl<key128>(b, nSlabs) : kasa_build_impl::finish_begin_impl<uint64_t>(b, nSlabs))
}

extern "C" int kasa_build_slab(kasa_builder *b, uint64_t slab, uint64_t *nRecords, uint64_t *nTrie)
{
    KASA_GUARDED(kasa_build_impl::build_slab_impl(b, slab, nRecords, nTrie))
}

extern "C" int kasa_build_fetch_slab(kasa_builder *b, uint64_t first, uint64_t count, void *records, uint32_t *triePrefix, uint64_t *trieCount)
{
    KASA_GUARDED(kasa_build_impl::build_fetch_slab_impl(b, first, count, records, triePrefix, trieCount))
}

extern "C" int kasa_build_finish_end(kasa_builder *b, uint64_t *nRecords, uint64_t *nTrie)
{
    KASA_GUARDED(kasa_build_impl::build_finish_end_impl(b, nRecords, nTrie))
}

extern "C" int kasa_build_spill_stats(kasa_builder *b, uint64_t *stats8)
{
    if (!b || !stats8) return fail(KASA_E_ARG, "kasa_build_spill_stats: NULL argument");
    stats8[0] = b->spillRuns; stats8[1] = b->spillRecords;
    stats8[2] = b->spilled && b->state != kasa_builder::ADDING ? b->plan.slabs.size() : 0;
    stats8[3] = b->spilled ? b->plan.largestSlab : 0;
    stats8[4] = b->spilled ? b->plan.heaviestCount : 0;
    stats8[5] = b->spilled ? (uint64_t)(b->usUp + 0.5) : 0; stats8[6] = b->spilled ? (uint64_t)(b->usDown + 0.5) : 0; stats8[7] = 0;
    return KASA_OK;
}
