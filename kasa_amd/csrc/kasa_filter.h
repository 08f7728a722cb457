// kasa_filter.h -- the two files of --filter, split on the device, behind kasa_batch_filter* / kasa_filter_split of include/kasa_hip.h.
//
// Specification: filterReads of kasa_amd/host/kasa_identify.cpp.  Every read's record text (kasa_pool_keep_records: its
// non-empty lines, one line feed each) goes to side 0 (clean, flag 0) or side 1 (contaminants), in the reads' order.
//   records : the batch's record text back to back        recOff : u64[nReads + 1], from 0        flags : u8[nReads]
// Kernels, all streaming:
//   flt_mark_kernel : one lane per read: {1, the record's size} if flagged, else {0, 0}
//   two running sums (rocPRIM) over those: flagged reads and flagged bytes BEFORE every read.  They serve both sides: the
//                     clean reads before read r are r less the flagged ones, the clean bytes recOff[r] less the flagged ones
//   flt_list_kernel : one lane per read: its entry (source offset, output offset) in the list of its side, in order
//   the copy        : pair_gather_kernel<FilterOffsets> (kasa_parse.h), split by OUTPUT bytes, 64-bit positions, no atomics
// With gzip every wanted side's text then goes through bgzf_stream (the members of kasa_batch_bgzf, the context's code).
#pragma once

namespace kasa_filter {

using kasa_parse_impl::TILE_BYTES;
using kasa_parse_impl::WAVES;

// the entries of one side: entry j = records[src[j] ...) goes to output bytes [dst[j], dst[j + 1]); dst[n] = total
struct FilterOffsets {
    const uint64_t *s, *d;
    __device__ __forceinline__ uint64_t dst(uint64_t j) const { return d[j]; }
    __device__ __forceinline__ uint64_t src(uint64_t j) const { return s[j]; }
    __device__ __forceinline__ const uint8_t *base(uint64_t, const uint8_t *src1, const uint8_t *) const { return src1; }
    __device__ __forceinline__ uint64_t find(uint64_t lo, uint64_t hi, uint64_t o) const
    {
        while (lo < hi) { const uint64_t mid = lo + ((hi - lo + 1) >> 1); if (d[mid] <= o) lo = mid; else hi = mid - 1; }
        return lo;
    }
};

// one lane per read and one for the end (0, 0: the running sums' totals land there)
__global__ void flt_mark_kernel(const uint64_t *__restrict__ recOff, const uint8_t *__restrict__ flags, uint64_t n, uint64_t *__restrict__ cnt, uint64_t *__restrict__ byt)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    const bool f = r < n && flags[r] != 0;
    cnt[r] = f ? 1 : 0;
    byt[r] = f ? recOff[r + 1] - recOff[r] : 0;
}

// after the running sums.  A side that is not wanted has NULL lists.
__global__ void flt_list_kernel(const uint64_t *__restrict__ recOff, const uint8_t *__restrict__ flags, uint64_t n, const uint64_t *__restrict__ cnt, const uint64_t *__restrict__ byt,
                                uint64_t *__restrict__ src0, uint64_t *__restrict__ dst0, uint64_t *__restrict__ src1, uint64_t *__restrict__ dst1)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    const uint64_t c1 = cnt[r], b1 = byt[r], at = recOff[r];
    if (r == n) { if (dst0) dst0[n - c1] = at - b1; if (dst1) dst1[c1] = b1; return; }
    if (flags[r] != 0) { if (dst1) { src1[c1] = at; dst1[c1] = b1; } }
    else if (dst0) { src0[r - c1] = at; dst0[r - c1] = at - b1; }
}

struct SplitBufs { DevBuf *cnt, *byt, *src[2], *dst[2], *out[2], *scanTmp; };

// records, recOff (recOff[0] = 0), flags: device.  The wanted sides' texts land in b.out[side] (16-byte aligned), their sizes and
// reads in nBytes / nReads; returns with the stream idle.
static int split(hipStream_t stream, const uint8_t *records, const uint64_t *recOff, uint64_t n, const uint8_t *flags, unsigned sides, const SplitBufs &b,
                 uint64_t nBytes[2], uint64_t nReads[2])
{
    nBytes[0] = nBytes[1] = 0; nReads[0] = nReads[1] = 0;
    if (n == 0 || !(sides & 3u)) return KASA_OK;
    int rc;
    if ((rc = b.cnt->reserve((n + 1) * 8)) || (rc = b.byt->reserve((n + 1) * 8))) return rc;
    for (int s = 0; s < 2; ++s)
        if ((sides >> s) & 1u) { if ((rc = b.src[s]->reserve((n + 1) * 8)) || (rc = b.dst[s]->reserve((n + 1) * 8))) return rc; }
    uint64_t *cnt = b.cnt->as<uint64_t>(), *byt = b.byt->as<uint64_t>();
    flt_mark_kernel<<<blocks_for(n + 1, 256), 256, 0, stream>>>(recOff, flags, n, cnt, byt);
    HIPCHK(hipGetLastError());
    if ((rc = dev_exclusive_scan(*b.scanTmp, stream, cnt, cnt, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>())) ||
        (rc = dev_exclusive_scan(*b.scanTmp, stream, byt, byt, (uint64_t)0, (size_t)n + 1, rocprim::plus<uint64_t>()))) return rc;
    uint64_t *src[2], *dst[2];
    for (int s = 0; s < 2; ++s) { const bool on = (sides >> s) & 1u; src[s] = on ? b.src[s]->as<uint64_t>() : nullptr; dst[s] = on ? b.dst[s]->as<uint64_t>() : nullptr; }
    flt_list_kernel<<<blocks_for(n + 1, 256), 256, 0, stream>>>(recOff, flags, n, cnt, byt, src[0], dst[0], src[1], dst[1]);
    HIPCHK(hipGetLastError());
    uint64_t c1 = 0, b1 = 0, all = 0;
    if ((rc = fetch_async(stream, c1, cnt + n)) || (rc = fetch_async(stream, b1, byt + n)) || (rc = fetch(stream, all, recOff + n))) return rc;
    const uint64_t reads[2] = {n - c1, c1}, bytes[2] = {all - b1, b1};
    for (int s = 0; s < 2; ++s) {
        if (!((sides >> s) & 1u)) continue;
        nReads[s] = reads[s]; nBytes[s] = bytes[s];
        if (reads[s] == 0 || bytes[s] == 0) continue;
        if ((rc = b.out[s]->reserve(bytes[s] + 64))) return rc;
        if ((rc = kasa_parse_impl::gather64(records, nullptr, FilterOffsets{src[s], dst[s]}, reads[s], bytes[s], b.out[s]->as<uint8_t>(), stream))) return rc;
    }
    HIPCHK(hipStreamSynchronize(stream));
    return KASA_OK;
}

static int batch_filter_impl(kasa_ctx *c, const uint8_t *contaminated, unsigned sides, int gzip, uint64_t nBytes[2], uint64_t nReads[2])
{
    if (!c || !nBytes || !nReads) return fail(KASA_E_ARG, "kasa_batch_filter: NULL argument");
    if (sides & ~3u) return fail(KASA_E_ARG, "kasa_batch_filter: sides is a mask of bit 0 (clean) and bit 1 (contaminants)");
    if (!c->fltHaveRecords) return fail(KASA_E_STATE, "kasa_batch_filter: this batch has no records (kasa_parse_take from a pool with kasa_pool_keep_records)");
    if (!contaminated && !c->txtValid) return fail(KASA_E_STATE, "kasa_batch_filter: no flags of this batch (kasa_batch_text, or a host array)");
    HIPCHK(hipSetDevice(c->ix->device));
    c->fltValid = false; c->fltBytes[0] = c->fltBytes[1] = 0; c->fltGzip = gzip != 0;
    const uint64_t n = (uint64_t)c->nReads;
    const uint8_t *flags = c->txtFlags.as<uint8_t>();
    int rc;
    if (contaminated && n) {
        if ((rc = c->fltFlags.reserve(n + 64))) return rc;
        HIPCHK(hipMemcpyAsync(c->fltFlags.p, contaminated, n, hipMemcpyHostToDevice, c->stream));
        flags = c->fltFlags.as<uint8_t>();
    }
    const SplitBufs b = {&c->fltCnt, &c->fltByt, {&c->fltSrc[0], &c->fltSrc[1]}, {&c->fltDst[0], &c->fltDst[1]}, {&c->fltOut[0], &c->fltOut[1]}, &c->scanTmp};
    if ((rc = split(c->stream, c->fltRecords.as<uint8_t>(), c->fltRecOff.as<uint64_t>(), n, flags, sides, b, nBytes, nReads))) return rc;
    for (int s = 0; s < 2; ++s) {
        c->fltBytes[s] = nBytes[s];
        if (!gzip || nBytes[s] == 0) continue;
        uint64_t total = 0, nBlocks = 0;
        if ((rc = bgzf_stream("kasa_batch_filter", c->bgzCodeKind, c->fltOut[s].as<uint8_t>(), nBytes[s], c->bgzMembers, c->bgzSize, c->bgzOff, c->scanTmp, c->fltZ[s], c->bgzCode, c->stream, &total, &nBlocks))) return rc;
        c->fltBytes[s] = nBytes[s] = total;
    }
    c->fltValid = true;
    return KASA_OK;
}

static int split_tap_impl(int device, const char *records, const uint64_t *recOff, uint64_t n, const uint8_t *flags, int side, char *out, uint64_t cap, uint64_t *nOut, uint64_t *nReadsOut)
{
    if (!nOut || !nReadsOut || (n && (!recOff || !flags))) return fail(KASA_E_ARG, "kasa_filter_split: NULL argument");
    if (side != 0 && side != 1) return fail(KASA_E_ARG, "kasa_filter_split: side is 0 (clean) or 1 (contaminants)");
    *nOut = 0; *nReadsOut = 0;
    if (n == 0) return KASA_OK;
    if (recOff[0] != 0) return fail(KASA_E_ARG, "kasa_filter_split: recOff does not start at 0");
    for (uint64_t r = 0; r < n; ++r) if (recOff[r + 1] < recOff[r]) return fail(KASA_E_ARG, "kasa_filter_split: recOff descends at read %llu", (unsigned long long)r);
    if (recOff[n] && !records) return fail(KASA_E_ARG, "kasa_filter_split: NULL records");
    HIPCHK(hipSetDevice(device));
    ScopedBuf dRec, dOff, dFlags, cnt, byt, src[2], dst[2], o[2], scanTmp;
    int rc;
    if ((rc = dRec.reserve(recOff[n] + 64)) || (rc = dOff.reserve((n + 1) * 8)) || (rc = dFlags.reserve(n + 64))) return rc;
    if (recOff[n]) HIPCHK(hipMemcpy(dRec.p, records, recOff[n], hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dOff.p, recOff, (n + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dFlags.p, flags, n, hipMemcpyHostToDevice));
    const SplitBufs b = {&cnt, &byt, {&src[0], &src[1]}, {&dst[0], &dst[1]}, {&o[0], &o[1]}, &scanTmp};
    uint64_t nb[2], nr[2];
    if ((rc = split(nullptr, dRec.as<uint8_t>(), dOff.as<uint64_t>(), n, dFlags.as<uint8_t>(), 1u << side, b, nb, nr))) return rc;
    *nOut = nb[side]; *nReadsOut = nr[side];
    if (nb[side] > cap) return fail(KASA_E_LIMIT, "kasa_filter_split: the side has %llu bytes, the destination takes %llu", (unsigned long long)nb[side], (unsigned long long)cap);
    if (nb[side] && !out) return fail(KASA_E_ARG, "kasa_filter_split: NULL destination");
    if (nb[side]) HIPCHK(hipMemcpy(out, o[side].p, nb[side], hipMemcpyDeviceToHost));
    return KASA_OK;
}

}  // namespace kasa_filter

extern "C" int kasa_batch_filter(kasa_ctx *ctx, const uint8_t *contaminated, unsigned sides, int gzip, uint64_t nBytes[2], uint64_t nReads[2])
{
    KASA_GUARDED(kasa_filter::batch_filter_impl(ctx, contaminated, sides, gzip, nBytes, nReads))
}

extern "C" int kasa_batch_filter_fetch_range(kasa_ctx *c, int side, void *dst, uint64_t offset, uint64_t nBytes)
{
    if (!c) return fail(KASA_E_ARG, "kasa_batch_filter_fetch_range: NULL argument");
    if (side != 0 && side != 1) return fail(KASA_E_ARG, "kasa_batch_filter_fetch_range: side is 0 (clean) or 1 (contaminants)");
    if (!c->fltValid) return fail(KASA_E_STATE, "kasa_batch_filter_fetch_range: no split of this batch (kasa_batch_filter)");
    if (offset > c->fltBytes[side] || nBytes > c->fltBytes[side] - offset)
        return fail(KASA_E_ARG, "kasa_batch_filter_fetch_range: beyond the side's %llu bytes", (unsigned long long)c->fltBytes[side]);
    if (nBytes && !dst) return fail(KASA_E_ARG, "kasa_batch_filter_fetch_range: NULL destination");
    HIPCHK(hipSetDevice(c->ix->device));
    const DevBuf &from = c->fltGzip ? c->fltZ[side] : c->fltOut[side];
    if (nBytes) HIPCHK(hipMemcpyAsync(dst, from.as<char>() + offset, nBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KASA_OK;
}

extern "C" int kasa_filter_split(int device, const char *records, const uint64_t *recOff, uint64_t nReads, const uint8_t *flags, int side, char *out, uint64_t cap,
                                 uint64_t *nOut, uint64_t *nReadsOut)
{
    KASA_GUARDED(kasa_filter::split_tap_impl(device, records, recOff, nReads, flags, side, out, cap, nOut, nReadsOut))
}
