// kasa_edit.h -- `kASA update | delete | shrink | getFrequency` on the device, behind kasa_build_add_index / drop_taxa / shrink
// of include/kasa_hip.h.  An existing index is one more sorted run of the builder (kasa_build.h): the finish merges it once
// with the brick runs' result, then the filters drop records, then the builder's emit, trie and frequency kernels run as for
// a build.
//
// Reference: Update.hpp:28-180 (update = sorted union with the records `build` makes, delete = the records of the taxa not
// listed), Shrink.hpp:152-370 (every n-th record of a taxon, the entropy of a k-mer, the halved 6-byte index).  Here:
//   load    : packed file records -> (key, rank), the rank by binary search of the tax ID; the same pass checks strict
//             (k-mer, tax ID) order, across chunk boundaries too.  A bad record is reported by the first index in a device
//             word (atomicMin), never by a trap.                                                        [edit_load_kernel]
//   delete  : a per-rank drop mask -> flags -> running sum -> scatter                      [edit_drop_flag, edit_scatter]
//   nth     : the ordinal of every record within its taxon in index order: per chunk of < 2^32 records a stable radix sort of
//             (rank, chunk index), the ordinal = place - start of the rank + the rank's count in earlier chunks; dropped iff
//             the ordinal is in the host's table {floor(d_m)} (a bitmap)             [edit_rank_hist, edit_nth_flag, edit_carry]
//   entropy : the multiplicity of every distinct letter of a k-mer as a popcount, the normalised Shannon entropy in double
//                                                                                                      [edit_entropy_flag]
//   halved  : kept iff the six low letters (bits 0-29) are not all '^'; 6-byte records {u32 low 30 bits, u16 content row}
//                                                                                         [edit_half_flag, edit_emit_half]
//   taxa    : after the finish, over the packed file records: how many distinct k-mers carry exactly c records (redundancy,
//             Shrink.hpp:35-72).  A record that opens a k-mer's run contributes its index to a running maximum (rocPRIM), so
//             every record knows where its run began; the run's last record adds one to the bin of its length
//                                                                                              [EditHeadPos, edit_taxa_hist]
// Positions are 64-bit: an edited index may hold more than 2^32 records.
#pragma once
#include <cmath>

namespace kasa_build_impl {

static constexpr uint64_t EDIT_CHUNK = 1ull << 30;     // records per radix sort of the nth filter (< 2^32)

// rec[j * W, (j + 1) * W) for j < count -> k[first + j], v[first + j]; reads k/v[first - 1] (written by the previous chunk)
template <class Key>
__global__ void edit_load_kernel(const uint32_t *__restrict__ rec, uint64_t first, uint64_t count, const uint32_t *__restrict__ idOfRank, uint32_t nRank,
                                 Key *__restrict__ k, uint32_t *__restrict__ v, unsigned long long *__restrict__ err)
{
    constexpr int W = sizeof(Key) / 4 + 1;
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < count; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t *r = rec + j * W;
        Key x = 0;
#pragma unroll
        for (int w = 0; w < W - 1; ++w) x |= (Key)r[w] << (32 * w);
        const uint32_t tid = r[W - 1];
        uint32_t lo = 0, hi = nRank;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (idOfRank[mid] < tid) lo = mid + 1; else hi = mid; }
        bool bad = lo >= nRank || idOfRank[lo] != tid;
        const uint64_t i = first + j;
        if (i > 0) {
            Key pk = 0; uint32_t pt;
            if (j > 0) {
                const uint32_t *q = r - W;
#pragma unroll
                for (int w = 0; w < W - 1; ++w) pk |= (Key)q[w] << (32 * w);
                pt = q[W - 1];
            } else { pk = k[i - 1]; pt = idOfRank[v[i - 1]]; }
            if (!pair_less<Key>(pk, pt, x, tid)) bad = true;
        }
        k[i] = x; v[i] = bad ? 0u : lo;
        if (bad) atomicMin(err, (unsigned long long)i);
    }
}

__global__ void edit_drop_flag_kernel(const uint32_t *__restrict__ v, uint64_t n, const uint8_t *__restrict__ drop, uint32_t *__restrict__ f)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        f[i] = drop[v[i]] ? 0u : 1u;
}

// halved (Shrink.hpp:78-143): an entry whose six low letters are all '^' goes (Shrink.hpp:108 compares the low 30 bits with
// that one value); a '^' at letter 5 over a real letter below it -- amino-acid input may hold '^' or '~' -- stays
static constexpr uint32_t HALF_SIX_PADS = 30u * ((1u << 25) | (1u << 20) | (1u << 15) | (1u << 10) | (1u << 5) | 1u);   // 1039104990
template <class Key>
__global__ void edit_half_flag_kernel(const Key *__restrict__ k, uint64_t n, uint32_t *__restrict__ f)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        f[i] = ((uint32_t)k[i] & 0x3FFFFFFFu) != HALF_SIX_PADS ? 1u : 0u;
}

// entropy (Shrink.hpp:152-236): H = -sum over the distinct letters (c / K) log2(c / K), '^' included; kept iff H ln2 / ln22 > 0.5.
// A letter's multiplicity is a popcount: every 5-bit field of x XOR (the letter in every field) that is zero.  The reference sums
// float terms in double; no multiset of 12 or 25 letters lies close enough to the threshold for the two to decide differently
// (tests/test_gpu_edit.py checks every partition).
__device__ __forceinline__ int popc_key(uint64_t x) { return __popcll(x); }
__device__ __forceinline__ int popc_key(key128 x) { return __popcll((uint64_t)x) + __popcll((uint64_t)(x >> 64)); }
template <class Key>
__global__ __launch_bounds__(256) void edit_entropy_flag_kernel(const Key *__restrict__ k, uint64_t n, uint32_t *__restrict__ f)
{
    constexpr int KL = KeyTraits<Key>::LETTERS;
    constexpr Key ONES = field_repeat<Key>(1u);
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const Key x = k[i];
        uint32_t seen = 0;
        double h = 0.0;
#pragma unroll 1
        for (int j = 0; j < KL; ++j) {
            const uint32_t c = (uint32_t)(x >> (5 * j)) & 31u;
            if ((seen >> c) & 1u) continue;
            seen |= 1u << c;
            const Key y = x ^ (ONES * (Key)c);
            const Key z = ~(y | (y >> 1) | (y >> 2) | (y >> 3) | (y >> 4)) & ONES;
            const double p = (double)popc_key(z) / KL;
            h -= p * log2(p);
        }
        f[i] = h * 0.69314718055994530942 / 3.09104245335831585347 > 0.5 ? 1u : 0u;   // ln 2, ln 22
    }
}

// hist[rank] += records of the rank in v[0, n); LDS: counters of every rank privatised per block (nRank <= FREQ_LDS_CELLS)
template <bool LDS>
__global__ __launch_bounds__(256) void edit_rank_hist_kernel(const uint32_t *__restrict__ v, uint64_t n, uint32_t nRank, unsigned long long *__restrict__ hist)
{
    __shared__ uint32_t sh[LDS ? FREQ_LDS_CELLS : 1];
    if (LDS) { for (uint32_t i = threadIdx.x; i < nRank; i += blockDim.x) sh[i] = 0u; __syncthreads(); }
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (LDS) atomicAdd(&sh[v[i]], 1u);
        else atomicAdd(&hist[v[i]], 1ull);
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nRank; i += blockDim.x) if (sh[i]) atomicAdd(&hist[i], (unsigned long long)sh[i]);
    }
}

__global__ void edit_iota_kernel(uint32_t *__restrict__ out, uint64_t m)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x) out[i] = (uint32_t)i;
}

// the chunk sorted by rank (sr: ranks, si: chunk indices): the record at place p is the (carry[r] + p - start[r] + 1)-th of its
// taxon; dropped iff that ordinal's bit is set in drop[0, nBits).  Writes f[si[p]], si[p] < m.
__global__ void edit_nth_flag_kernel(const uint32_t *__restrict__ sr, const uint32_t *__restrict__ si, uint64_t m, const uint64_t *__restrict__ start,
                                     const unsigned long long *__restrict__ carry, const uint32_t *__restrict__ drop, uint64_t nBits, uint32_t *__restrict__ f)
{
    for (uint64_t p = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; p < m; p += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = sr[p];
        const uint64_t ord = carry[r] + (p - start[r]) + 1;
        const bool gone = ord < nBits && ((drop[ord >> 5] >> (ord & 31)) & 1u);
        f[si[p]] = gone ? 0u : 1u;
    }
}

__global__ void edit_carry_kernel(unsigned long long *__restrict__ carry, const unsigned long long *__restrict__ chunk, uint32_t nRank)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nRank) carry[r] += chunk[r];
}

template <class Key>
__global__ void edit_scatter_kernel(const Key *__restrict__ k, const uint32_t *__restrict__ v, uint64_t n, const uint32_t *__restrict__ f,
                                    const uint64_t *__restrict__ pos, Key *__restrict__ ko, uint32_t *__restrict__ vo)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (f[i]) { ko[pos[i]] = k[i]; vo[pos[i]] = v[i]; }
}

// 6-byte records of the halved index as three u16 words: low 30 bits of the k-mer (low half, high half), the content row
template <class Key>
__global__ void edit_emit_half_kernel(const Key *__restrict__ k, const uint32_t *__restrict__ v, uint64_t n, const uint32_t *__restrict__ rowOfRank,
                                      uint16_t *__restrict__ rec)
{
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t low = (uint32_t)k[i] & 0x3FFFFFFFu;
        rec[3 * i] = (uint16_t)low; rec[3 * i + 1] = (uint16_t)(low >> 16); rec[3 * i + 2] = (uint16_t)rowOfRank[v[i]];
    }
}

// records i and j of the packed file records carry the same k-mer
template <class Key>
__host__ __device__ __forceinline__ bool edit_same_kmer(const uint32_t *__restrict__ rec, uint64_t i, uint64_t j)
{
    constexpr int W = sizeof(Key) / 4 + 1;
    bool same = true;
#pragma unroll
    for (int w = 0; w < W - 1; ++w) same &= rec[i * W + w] == rec[j * W + w];
    return same;
}
// i where record i opens the run of a k-mer, 0 elsewhere: the running maximum is the index of the run's first record
template <class Key>
struct EditHeadPos {
    const uint32_t *rec;
    __host__ __device__ uint64_t operator()(uint64_t i) const { return (i == 0 || !edit_same_kmer<Key>(rec, i, i - 1)) ? i : 0; }
};

// hist[c] += k-mers with exactly c records, c < nBins.  The last record of a run knows the run's length from head[i].  Nearly every
// run has length 1: those are counted in a register and summed per wavefront; lengths below TAXA_LDS_BINS go to LDS bins that the
// block flushes once; longer runs (a crowded index has few) add to the global bins directly.  A run of nBins records or more is
// reported by the index of its last record in a device word (atomicMin).  Reads rec[0, n * W), head[0, n); writes hist[0, nBins).
static constexpr int TAXA_LDS_BINS = 1024;
template <class Key>
__global__ __launch_bounds__(256) void edit_taxa_hist_kernel(const uint32_t *__restrict__ rec, const uint64_t *__restrict__ head, uint64_t n, uint64_t nBins,
                                                             unsigned long long *__restrict__ hist, unsigned long long *__restrict__ err)
{
    __shared__ uint32_t sh[TAXA_LDS_BINS];
    for (uint32_t c = threadIdx.x; c < TAXA_LDS_BINS; c += blockDim.x) sh[c] = 0u;
    __syncthreads();
    uint32_t ones = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i + 1 < n && edit_same_kmer<Key>(rec, i, i + 1)) continue;
        const uint64_t len = i - head[i] + 1;
        if (len >= nBins) atomicMin(err, (unsigned long long)i);
        else if (len == 1) ++ones;
        else if (len < (uint64_t)TAXA_LDS_BINS) atomicAdd(&sh[len], 1u);
        else atomicAdd(&hist[len], 1ull);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ones += __shfl_down(ones, off);
    if ((threadIdx.x & 63) == 0 && ones) atomicAdd(&sh[1], ones);
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < TAXA_LDS_BINS; c += blockDim.x)
        if (sh[c] && c < nBins) atomicAdd(&hist[c], (unsigned long long)sh[c]);
}

template <class Key>
static int taxa_histogram(kasa_builder *b, uint64_t *hist, uint64_t nBins, uint64_t *distinctKmers)
{
    const uint64_t n = b->result.n;
    std::fill(hist, hist + nBins, (uint64_t)0);
    *distinctKmers = 0;
    if (n == 0) return KASA_OK;
    int rc;
    DevBuf head, bins;
    if ((rc = head.reserve(n * 8 + 64)) || (rc = bins.reserve(nBins * 8 + 64)) || (rc = b->loadErr.reserve(64))) return rc;
    const uint32_t *rec = b->rec.as<uint32_t>();
    unsigned long long *err = b->loadErr.as<unsigned long long>(), *d = bins.as<unsigned long long>();
    unsigned long long bad = ~0ull;
    HIPCHK(hipMemcpyAsync(err, &bad, 8, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemsetAsync(d, 0, nBins * 8, b->stream));
    rocprim::transform_iterator<rocprim::counting_iterator<uint64_t>, EditHeadPos<Key>, uint64_t> in(rocprim::counting_iterator<uint64_t>(0), EditHeadPos<Key>{rec});
    if ((rc = dev_inclusive_scan(b->scanTmp, b->stream, in, head.as<uint64_t>(), (size_t)n, rocprim::maximum<uint64_t>()))) return rc;
    edit_taxa_hist_kernel<Key><<<grid_for(n, 256, 1024), 256, 0, b->stream>>>(rec, head.as<uint64_t>(), n, nBins, d, err);
    HIPCHK(hipGetLastError());
    if ((rc = fetch_async(b->stream, bad, err))) return rc;
    HIPCHK(hipMemcpyAsync(hist, d, nBins * 8, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));                          // (head and bins go out of scope here)
    if (bad != ~0ull) {
        std::fill(hist, hist + nBins, (uint64_t)0);
        return fail(KASA_E_ARG, "kasa_build_taxa_histogram: the k-mer that ends at record %llu carries %llu records or more; pass nBins = taxa + 1", bad, (unsigned long long)nBins);
    }
    for (uint64_t c = 0; c < nBins; ++c) *distinctKmers += hist[c];
    return KASA_OK;
}

// the records of b->result with f[i] = 1, in order, become b->result
template <class Key>
static int compact_result(kasa_builder *b, const uint32_t *f)
{
    const uint64_t n = b->result.n;
    if (n == 0) return KASA_OK;
    int rc;
    DevBuf pos;
    if ((rc = pos.reserve(n * 8 + 64))) return rc;
    uint64_t *p = pos.as<uint64_t>();
    uint64_t nu = 0;
    if ((rc = flag_places(b, f, n, p, nu))) return rc;
    if (nu == n) return KASA_OK;
    kasa_builder::Run out;
    if ((rc = out.k.reserve(nu * sizeof(Key) + 64)) || (rc = out.v.reserve(nu * 4 + 64))) return rc;
    edit_scatter_kernel<Key><<<grid_for(n), 256, 0, b->stream>>>(b->result.k.as<Key>(), b->result.v.as<uint32_t>(), n, f, p, out.k.as<Key>(), out.v.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));
    out.n = nu;
    b->result = std::move(out);
    return KASA_OK;
}

// deleteEveryNth (Shrink.hpp:270-308): a taxon's j-th record (j = 1, 2, ...) goes iff j == (uint64_t)d for the current d, and d
// advances by step = 100 / |P| (double) on every drop, d_1 = step.  With step >= 1 that is membership of j in the increasing
// table {(uint64_t)d_m}, the same for every taxon; with step < 1 (or P = 0) the first threshold, 0, is never met.  Bit j of the
// result for j <= maxOrd.
static std::vector<uint32_t> nth_drop_bitmap(float P, uint64_t maxOrd)
{
    std::vector<uint32_t> bits((size_t)(maxOrd / 32 + 1), 0u);
    const float a = fabsf(P);
    if (a == 0.f) return bits;
    const double step = 100. / a;
    if (!(step >= 1.0)) return bits;
    for (double d = step; d < 1.8e19 && (uint64_t)d <= maxOrd; d += step) {
        const uint64_t j = (uint64_t)d;
        bits[(size_t)(j >> 5)] |= 1u << (j & 31);
    }
    return bits;
}

template <class Key>
static int nth_flags(kasa_builder *b, uint32_t *f)
{
    const uint64_t n = b->result.n;
    const uint32_t nRank = (uint32_t)b->ids.size();
    const uint32_t *v = b->result.v.as<uint32_t>();
    int rc;
    const bool lds = nRank <= (uint32_t)FREQ_LDS_CELLS;
    auto hist = [&](const uint32_t *x, uint64_t m, unsigned long long *h) {
        if (lds) edit_rank_hist_kernel<true><<<grid_for(m, 256, 1024), 256, 0, b->stream>>>(x, m, nRank, h);
        else edit_rank_hist_kernel<false><<<grid_for(m, 256, 8192), 256, 0, b->stream>>>(x, m, nRank, h);
    };
    // the largest taxon sizes the table
    DevBuf total, carry, chunkH, start;
    if ((rc = total.reserve((size_t)nRank * 8 + 64)) || (rc = carry.reserve((size_t)nRank * 8 + 64)) || (rc = chunkH.reserve((size_t)nRank * 8 + 64)) ||
        (rc = start.reserve((size_t)nRank * 8 + 64)))
        return rc;
    unsigned long long *tot = total.as<unsigned long long>(), *car = carry.as<unsigned long long>(), *ch = chunkH.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(tot, 0, (size_t)nRank * 8, b->stream));
    HIPCHK(hipMemsetAsync(car, 0, (size_t)nRank * 8, b->stream));
    hist(v, n, tot);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> hTot(nRank);
    HIPCHK(hipMemcpyAsync(hTot.data(), tot, (size_t)nRank * 8, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    const uint64_t maxOrd = *std::max_element(hTot.begin(), hTot.end());
    const std::vector<uint32_t> bits = nth_drop_bitmap(b->shrinkP, maxOrd);
    DevBuf dBits;
    if ((rc = dBits.reserve(bits.size() * 4 + 64))) return rc;
    HIPCHK(hipMemcpyAsync(dBits.p, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, b->stream));
    // chunks of < 2^32 records (KASA_EDIT_CHUNK_RECORDS: smaller chunks, so that tests reach the carry between them)
    uint64_t chunk = EDIT_CHUNK;
    if (const char *e = getenv("KASA_EDIT_CHUNK_RECORDS")) chunk = std::max<uint64_t>(1, std::min<uint64_t>(EDIT_CHUNK, (uint64_t)atoll(e)));
    const uint64_t cm = std::min(chunk, n);
    DevBuf kA, vA, kB, vB, tmpSort;
    if ((rc = kA.reserve(cm * 4 + 64)) || (rc = vA.reserve(cm * 4 + 64)) || (rc = kB.reserve(cm * 4 + 64)) || (rc = vB.reserve(cm * 4 + 64)) ||
        (rc = tmpSort.reserve(kasa_radix::scratch_bytes<uint32_t>(cm))))
        return rc;
    auto starts = [&]() -> int {                                       // (every chunk scans nRank counts: the first call reserves)
        return dev_exclusive_scan(b->scanTmp, b->stream, ch, start.as<uint64_t>(), (uint64_t)0, (size_t)nRank, rocprim::plus<uint64_t>());
    };
    for (uint64_t c0 = 0; c0 < n; c0 += chunk) {
        const uint64_t m = std::min(chunk, n - c0);
        HIPCHK(hipMemcpyAsync(kA.p, v + c0, m * 4, hipMemcpyDeviceToDevice, b->stream));
        edit_iota_kernel<<<grid_for(m), 256, 0, b->stream>>>(vA.as<uint32_t>(), m);
        uint32_t *sr, *si;
        HIPCHK(kasa_radix::sort_pairs<uint32_t>(kA.as<uint32_t>(), vA.as<uint32_t>(), kB.as<uint32_t>(), vB.as<uint32_t>(), (uint32_t)m, 0, 24, tmpSort.p, b->stream, &sr, &si));
        HIPCHK(hipMemsetAsync(ch, 0, (size_t)nRank * 8, b->stream));
        hist(sr, m, ch);
        if ((rc = starts())) return rc;
        edit_nth_flag_kernel<<<grid_for(m), 256, 0, b->stream>>>(sr, si, m, start.as<uint64_t>(), car, dBits.as<uint32_t>(), (uint64_t)bits.size() * 32, f + c0);
        edit_carry_kernel<<<blocks_for(nRank, 256), 256, 0, b->stream>>>(car, ch, nRank);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(b->stream));                          // (the chunk buffers go out of scope here)
    return KASA_OK;
}

template <class Key>
static int edit_finish(kasa_builder *b)
{
    int rc;
    if (b->loading) return fail(KASA_E_STATE, "kasa_build_finish: the index run holds %llu of its %llu records", (unsigned long long)b->loadNext, (unsigned long long)b->loadTotal);
    {
        // every index run takes part in one merge, with the result of the bricks and the index runs before it
        StageClock clk(&b->ms[2], b->stream);
        for (kasa_builder::Run &r : b->idxRuns) {
            if (b->result.n == 0) { b->result = std::move(r); continue; }
            if (r.n == 0) continue;
            kasa_builder::Run m;
            if ((rc = merge_two<Key>(b, b->result, r, m))) return rc;
            r.k.release(); r.v.release();
            b->result = std::move(m);
        }
        b->idxRuns.clear();
        clk.stop();
    }
    const bool drop = std::find(b->dropRank.begin(), b->dropRank.end(), (uint8_t)1) != b->dropRank.end();
    if (!drop && !b->shrinkStrategy) return KASA_OK;
    StageClock clk(&b->msEdit, b->stream);
    const uint64_t n0 = b->result.n;
    if ((rc = b->flags.reserve(n0 * 4 + 64))) return rc;
    uint32_t *f = b->flags.as<uint32_t>();
    if (drop && n0) {
        DevBuf mask;
        if ((rc = mask.reserve(b->dropRank.size() + 64))) return rc;
        HIPCHK(hipMemcpyAsync(mask.p, b->dropRank.data(), b->dropRank.size(), hipMemcpyHostToDevice, b->stream));
        edit_drop_flag_kernel<<<grid_for(n0), 256, 0, b->stream>>>(b->result.v.as<uint32_t>(), n0, mask.as<uint8_t>(), f);
        HIPCHK(hipGetLastError());
        if ((rc = compact_result<Key>(b, f))) return rc;
    }
    b->droppedDelete = n0 - b->result.n;
    const uint64_t n1 = b->result.n;
    if (b->shrinkStrategy == 2) {                                     // the halved index keeps the frequency file of the full one
        if ((rc = freq_zero<Key>(b)) || (rc = freq_accumulate<Key>(b, b->result.k.as<Key>(), b->result.v.as<uint32_t>(), n1)) || (rc = freq_final<Key>(b))) return rc;
    }
    if (b->shrinkStrategy && n1) {
        const Key *k = b->result.k.as<Key>();
        if (b->shrinkStrategy == 1) { if ((rc = nth_flags<Key>(b, f))) return rc; }
        else if (b->shrinkStrategy == 2) edit_half_flag_kernel<Key><<<grid_for(n1), 256, 0, b->stream>>>(k, n1, f);
        else edit_entropy_flag_kernel<Key><<<grid_for(n1), 256, 0, b->stream>>>(k, n1, f);
        HIPCHK(hipGetLastError());
        if ((rc = compact_result<Key>(b, f))) return rc;
    }
    b->droppedShrink = n1 - b->result.n;
    if (b->shrinkStrategy && b->result.n == 0)
        return fail(KASA_E_ARG, "kasa_build_shrink: strategy %d leaves no record of the %llu", b->shrinkStrategy, (unsigned long long)n1);
    b->halved = b->shrinkStrategy == 2;
    clk.stop();
    return KASA_OK;
}

template <class Key>
static int edit_emit_halved(kasa_builder *b, const Key *k, const uint32_t *v, uint64_t n)
{
    std::vector<uint32_t> rowOfRank(b->ids.size(), 0u);
    for (size_t r = 0; r < b->rowRank.size(); ++r) if (b->rowRank[r] != ~0u) rowOfRank[b->rowRank[r]] = (uint32_t)r;
    DevBuf d;
    int rc;
    if ((rc = d.reserve(rowOfRank.size() * 4 + 64))) return rc;
    HIPCHK(hipMemcpyAsync(d.p, rowOfRank.data(), rowOfRank.size() * 4, hipMemcpyHostToDevice, b->stream));
    edit_emit_half_kernel<Key><<<grid_for(n), 256, 0, b->stream>>>(k, v, n, d.as<uint32_t>(), b->rec.as<uint16_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));                          // (d goes out of scope here)
    return KASA_OK;
}

} // namespace kasa_build_impl

static int build_add_index_impl(kasa_builder *b, uint64_t first, uint64_t count, uint64_t total, const void *records)
{
    using namespace kasa_build_impl;
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->state != kasa_builder::ADDING) return fail(KASA_E_STATE, "kasa_build_add_index: the build is finished");
    if (b->resident || b->spilled) return fail(KASA_E_STATE, "kasa_build_add_index: edits need the runs on the device (the builder has a resident budget or spilled runs)");
    b->edited = true;
    if (count && !records) return fail(KASA_E_ARG, "kasa_build_add_index: records is NULL");
    if (first > total || count > total - first)
        return fail(KASA_E_ARG, "kasa_build_add_index: records [%llu, +%llu) outside the run of %llu", (unsigned long long)first, (unsigned long long)count, (unsigned long long)total);
    HIPCHK(hipSetDevice(b->device));
    int rc;
    if (first == 0) {
        if (b->loading) return fail(KASA_E_STATE, "kasa_build_add_index: the index run before holds %llu of its %llu records", (unsigned long long)b->loadNext, (unsigned long long)b->loadTotal);
        kasa_builder::Run r;
        if ((rc = r.k.reserve(total * (uint64_t)b->keyBytes() + 64)) || (rc = r.v.reserve(total * 4 + 64))) return rc;
        b->idxRuns.push_back(std::move(r));
        b->loading = true; b->loadNext = 0; b->loadTotal = total;
    } else if (!b->loading || first != b->loadNext || total != b->loadTotal)
        return fail(KASA_E_ARG, "kasa_build_add_index: records from %llu of a run of %llu, expected %llu of %llu", (unsigned long long)first, (unsigned long long)total,
                    (unsigned long long)b->loadNext, (unsigned long long)b->loadTotal);
    kasa_builder::Run &run = b->idxRuns.back();
    const uint64_t recBytes = b->wide ? 20 : 12;
    if (count) {
        if ((rc = b->loadStage.reserve(count * recBytes + 64)) || (rc = b->loadErr.reserve(64))) return rc;
        unsigned long long bad = ~0ull;
        {
            StageClock clk(&b->msEdit, b->stream);
            HIPCHK(hipMemcpyAsync(b->loadStage.p, records, count * recBytes, hipMemcpyHostToDevice, b->stream));
            HIPCHK(hipMemcpyAsync(b->loadErr.p, &bad, 8, hipMemcpyHostToDevice, b->stream));
            const uint32_t *src = b->loadStage.as<uint32_t>();
            unsigned long long *err = b->loadErr.as<unsigned long long>();
            if (b->wide) edit_load_kernel<key128><<<grid_for(count), 256, 0, b->stream>>>(src, first, count, b->idOfRank.as<uint32_t>(), (uint32_t)b->ids.size(), run.k.as<key128>(), run.v.as<uint32_t>(), err);
            else edit_load_kernel<uint64_t><<<grid_for(count), 256, 0, b->stream>>>(src, first, count, b->idOfRank.as<uint32_t>(), (uint32_t)b->ids.size(), run.k.as<uint64_t>(), run.v.as<uint32_t>(), err);
            HIPCHK(hipGetLastError());
            if ((rc = fetch(b->stream, bad, err))) return rc;
            clk.stop();
        }
        if (bad != ~0ull) {
            const uint8_t *rec = static_cast<const uint8_t *>(records) + (bad - first) * recBytes;
            uint32_t tid; memcpy(&tid, rec + recBytes - 4, 4);
            const bool known = std::binary_search(b->ids.begin(), b->ids.end(), tid);
            b->loading = false; b->idxRuns.pop_back();
            if (!known) return fail(KASA_E_ARG, "kasa_build_add_index: record %llu has tax ID %u, which the content file does not list", (unsigned long long)bad, tid);
            return fail(KASA_E_ARG, "kasa_build_add_index: record %llu (tax ID %u) does not follow its predecessor in strict (k-mer, tax ID) order: the index is unsorted or holds a duplicate",
                        (unsigned long long)bad, tid);
        }
    }
    b->loadNext += count;
    b->indexIn += count;
    run.n = b->loadNext;
    if (b->loadNext == b->loadTotal) b->loading = false;
    return KASA_OK;
}

extern "C" int kasa_build_add_index(kasa_builder *b, uint64_t first, uint64_t count, uint64_t total, const void *records)
{
    KASA_GUARDED(build_add_index_impl(b, first, count, total, records))
}

static int build_drop_taxa_impl(kasa_builder *b, const uint32_t *taxIds, uint64_t n)
{
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->state != kasa_builder::ADDING) return fail(KASA_E_STATE, "kasa_build_drop_taxa: the build is finished");
    if (b->resident || b->spilled) return fail(KASA_E_STATE, "kasa_build_drop_taxa: edits need the runs on the device (the builder has a resident budget or spilled runs)");
    b->edited = true;
    if (n && !taxIds) return fail(KASA_E_ARG, "kasa_build_drop_taxa: taxIds is NULL");
    if (b->dropRank.empty()) b->dropRank.assign(b->ids.size(), 0);
    for (uint64_t i = 0; i < n; ++i) {                                 // IDs the content file does not list name no record
        const auto it = std::lower_bound(b->ids.begin(), b->ids.end(), taxIds[i]);
        if (it != b->ids.end() && *it == taxIds[i]) b->dropRank[(size_t)(it - b->ids.begin())] = 1;
    }
    return KASA_OK;
}

extern "C" int kasa_build_drop_taxa(kasa_builder *b, const uint32_t *taxIds, uint64_t n)
{
    KASA_GUARDED(build_drop_taxa_impl(b, taxIds, n))
}

extern "C" int kasa_build_shrink(kasa_builder *b, int strategy, float percentage)
{
    if (!b) return fail(KASA_E_ARG, "builder is NULL");
    if (b->state != kasa_builder::ADDING) return fail(KASA_E_STATE, "kasa_build_shrink: the build is finished");
    if (b->resident || b->spilled) return fail(KASA_E_STATE, "kasa_build_shrink: edits need the runs on the device (the builder has a resident budget or spilled runs)");
    b->edited = true;
    if (b->shrinkStrategy) return fail(KASA_E_STATE, "kasa_build_shrink: called twice");
    if (strategy < 1 || strategy > 3) return fail(KASA_E_ARG, "kasa_build_shrink: strategy must be 1 (every n-th k-mer of a taxon), 2 (halved) or 3 (entropy), got %d", strategy);
    if (strategy == 2 && b->wide) return fail(KASA_E_ARG, "kasa_build_shrink: If k is larger than 12, the index can not be halved as of now!");
    if (strategy == 2 && b->rowRank.size() > 65535)
        return fail(KASA_E_ARG, "kasa_build_shrink: Index can only be halved, if less than 65535 species are inside the index! (%zu content rows)", b->rowRank.size() - 1);
    if (strategy == 1 && !std::isfinite(percentage)) return fail(KASA_E_ARG, "kasa_build_shrink: the percentage is not a number");
    b->shrinkStrategy = strategy;
    b->shrinkP = percentage;
    return KASA_OK;
}

extern "C" int kasa_build_edit_stats(kasa_builder *b, uint64_t *stats4)
{
    if (!b || !stats4) return fail(KASA_E_ARG, "kasa_build_edit_stats: NULL argument");
    stats4[0] = b->indexIn; stats4[1] = b->droppedDelete; stats4[2] = b->droppedShrink;
    stats4[3] = (uint64_t)(b->msEdit * 1000.0 + 0.5);                  // device microseconds of the loads and the filters
    return KASA_OK;
}

static int build_taxa_histogram_impl(kasa_builder *b, uint64_t *hist, uint64_t nBins, uint64_t *distinctKmers)
{
    using namespace kasa_build_impl;
    if (!b || !hist || !distinctKmers || nBins == 0) return fail(KASA_E_ARG, "kasa_build_taxa_histogram: NULL argument or no bins");
    if (b->state == kasa_builder::ADDING) return fail(KASA_E_STATE, "kasa_build_taxa_histogram: kasa_build_finish first");
    if (b->records != kasa_builder::ON_DEVICE) return fail(KASA_E_STATE, "kasa_build_taxa_histogram: the records of a spilled build are not on the device");
    if (b->halved) return fail(KASA_E_STATE, "kasa_build_taxa_histogram: a halved index keeps 30 bits of a k-mer, its records do not tell k-mers apart");
    HIPCHK(hipSetDevice(b->device));
    return b->wide ? taxa_histogram<key128>(b, hist, nBins, distinctKmers) : taxa_histogram<uint64_t>(b, hist, nBins, distinctKmers);
}

extern "C" int kasa_build_taxa_histogram(kasa_builder *b, uint64_t *hist, uint64_t nBins, uint64_t *distinctKmers)
{
    KASA_GUARDED(build_taxa_histogram_impl(b, hist, nBins, distinctKmers))
}
