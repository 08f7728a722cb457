// kasa_parse.h -- FASTA / FASTQ text -> the reads of a batch, on the device, behind kasa_parse_* of include/kasa_hip.h.
//
// Specification: parseRecords of kasa_amd/host/kasa_identify.cpp (what Read.hpp:699-760 hands on for reads that fit one chunk).
// A chunk of whole records (it starts at a header line; only its last line may lack a line feed) becomes
//   bases   : the sequence lines back to back, untouched ('\r' stays, no cleaning, no case folding)
//   off     : running offsets into bases
//   names   : header without its first character + one space, back to back, with nameOff
//   lengths : letters + one per sequence line (FASTA: per non-empty sequence line)
// behind the reads the pool already holds.  Kernels, all streaming (bound: HBM copy rate):
//   line table : prs_count_kernel (16-byte loads, line feeds per tile of a wavefront), one running sum over the tiles
//                (rocPRIM), prs_lines_kernel (the same loads again, every line feed writes the start of the next line)
//   classify   : prs_classify_kernel, one lane per line: header / sequence line / neither, the FASTQ form checked line by
//                line; two running sums (rocPRIM) over {headers, sequence lines} and {sequence bytes, name bytes} give every
//                line its read, its place in `bases` and in `names`; prs_index_kernel lists the header lines and the
//                non-empty sequence lines; prs_reads_kernel, one lane per read, writes off / nameOff / lengths
//   gather     : prs_gather_kernel, work split by OUTPUT bytes: a wavefront owns 4 KiB of the output, finds the first and last
//                source line of that tile in the list (wave-uniform binary searches), every lane finds the line of its 16
//                output bytes between those two, reads them with unaligned dword loads + v_alignbyte (or byte by byte where
//                the 16 bytes span lines) and stores one aligned 16-byte vector.  The same sweep checks the sequence bytes
//                for ' ' and '\t'.  No atomics except the one that reports the first offence; no lane walks a record.
// kasa_pool_keep_records: the pool also keeps every read's RECORD TEXT (what --filter writes back: every non-empty line of the
// record and one line feed each) with running recOff: prs_recsize_kernel, one running sum over the lines, prs_recindex_kernel
// and prs_recoff_kernel list the non-empty lines, and the gather's third flavour copies them behind the pool's end.
// A chunk that is not in the form the device takes (KASA_PARSE_* codes) leaves the pool as it was: everything is written
// behind the pool's end and the sizes move only when the status word is clean.
#pragma once
#include <memory>

namespace kasa_parse_impl {

static constexpr int STEP_BYTES = 1024;                 // 64 lanes x 16 bytes: one load instruction of a wavefront
static constexpr int STEPS = 4;
static constexpr int TILE_BYTES = STEP_BYTES * STEPS;   // what one wavefront owns (input tile of the line table, output tile of the gather)
static constexpr int WAVES = 4;                         // per workgroup
static constexpr uint64_t MAX_CHUNK = 0xFFFF0000ull;    // positions in a chunk are 32-bit

// 0x80 in every byte of w that equals the pattern's byte (exact per byte: no borrow between bytes)
__device__ __forceinline__ uint32_t eq_bytes(uint32_t w, uint32_t pattern)
{
    const uint32_t x = w ^ pattern;
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return ~(t | x | 0x7F7F7F7Fu);
}
__device__ __forceinline__ unsigned long long status_key(uint32_t pos, int code) { return ((unsigned long long)pos << 8) | (unsigned)code; }

// text is padded with zero bytes up to a whole tile: every load is a full one and a pad byte is no line feed
__global__ __launch_bounds__(64 * WAVES) void prs_count_kernel(const uint4 *__restrict__ text, uint32_t nTiles, uint32_t *__restrict__ tileCnt)
{
    const uint32_t tile = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= nTiles) return;
    const uint4 *p = text + (size_t)tile * (TILE_BYTES / 16) + lane;
    uint32_t c = 0;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const uint4 v = p[s * 64];
        c += __popc(eq_bytes(v.x, 0x0A0A0A0Au)) + __popc(eq_bytes(v.y, 0x0A0A0A0Au)) + __popc(eq_bytes(v.z, 0x0A0A0A0Au)) + __popc(eq_bytes(v.w, 0x0A0A0A0Au));
    }
    for (int o = 32; o; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
    if (lane == 0) { tileCnt[tile] = c; if (tile == 0) tileCnt[nTiles] = 0; }
}

// lineStart[0] = 0, lineStart[k + 1] = position behind the k-th line feed; line i = text[lineStart[i], lineStart[i + 1] - 1).
// A last line without a line feed ends at nBytes: lineStart[nLines] = nBytes + 1.
__global__ __launch_bounds__(64 * WAVES) void prs_lines_kernel(const uint4 *__restrict__ text, uint32_t nTiles, const uint32_t *__restrict__ tileOff,
                                                               uint32_t *__restrict__ lineStart, uint32_t nLines, uint32_t nBytes, int trailingFeed)
{
    const uint32_t tile = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= nTiles) return;
    if (tile == 0 && lane == 0) { lineStart[0] = 0; if (!trailingFeed) lineStart[nLines] = nBytes + 1; }
    const uint4 *p = text + (size_t)tile * (TILE_BYTES / 16) + lane;
    uint32_t base = tileOff[tile];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const uint4 v = p[s * 64];
        uint32_t m[4] = {eq_bytes(v.x, 0x0A0A0A0Au), eq_bytes(v.y, 0x0A0A0A0Au), eq_bytes(v.z, 0x0A0A0A0Au), eq_bytes(v.w, 0x0A0A0A0Au)};
        const uint32_t c = __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
        uint32_t incl = c;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, d); if ((int)lane >= d) incl += t; }
        uint32_t k = base + incl - c;
        const uint32_t pos0 = tile * TILE_BYTES + s * STEP_BYTES + lane * 16;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            for (uint32_t mm = m[w]; mm; mm &= mm - 1) lineStart[1 + k++] = pos0 + w * 4 + ((__ffs((int)mm) - 1) >> 3) + 1;
        base += (uint32_t)__shfl((int)incl, 63);
    }
}

// One lane per line.  k1 = headers << 32 | counted sequence lines, k2 = sequence bytes << 32 | name bytes (a chunk is below
// 2^32 bytes, so neither half carries into the other under a running sum); entry nLines = 0: the sums' totals land there.
__global__ void prs_classify_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ lineStart, uint32_t nLines, int fasta, uint64_t longSeq,
                                    uint64_t *__restrict__ k1, uint64_t *__restrict__ k2, unsigned long long *__restrict__ status)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nLines) return;
    if (i == nLines) {
        k1[i] = 0; k2[i] = 0;
        if (!fasta && (nLines & 3u)) atomicMin(status, status_key(lineStart[nLines & ~3u], KASA_PARSE_FASTQ_LINES));
        return;
    }
    const uint32_t s = lineStart[i], len = lineStart[i + 1] - 1 - s;
    const uint8_t c0 = len ? text[s] : 0;
    bool hdr, seq;
    if (fasta) {
        hdr = len > 0 && c0 == '>';
        seq = len > 0 && !hdr;                                   // empty lines are skipped and not counted
    } else {
        const uint32_t m = i & 3u;
        hdr = m == 0; seq = m == 1;
        int bad = 0;
        if (len == 0) bad = KASA_PARSE_EMPTY_LINE;
        else if (m == 0 && c0 != '@') bad = KASA_PARSE_FASTQ_HEADER;
        else if (m == 1 && c0 == '+') bad = KASA_PARSE_FASTQ_SEQ_PLUS;     // the host parser would take it for the '+' line
        else if (m == 1 && (uint64_t)len >= longSeq) bad = KASA_PARSE_LONG;
        else if (m == 2 && c0 != '+') bad = KASA_PARSE_FASTQ_PLUS;
        else if (m == 3 && len != lineStart[i - 1] - 1 - lineStart[i - 2]) bad = KASA_PARSE_FASTQ_QUALITY;
        if (bad) atomicMin(status, status_key(s, bad));
    }
    k1[i] = ((uint64_t)(hdr ? 1 : 0) << 32) | (uint64_t)(seq ? 1 : 0);
    k2[i] = ((uint64_t)(seq ? len : 0) << 32) | (uint64_t)(hdr ? len : 0);      // a name is the header less one character plus one space
}

// after the running sums: the header lines by read, the non-empty sequence lines in order with their place in the output
__global__ void prs_index_kernel(const uint32_t *__restrict__ lineStart, const uint64_t *__restrict__ k1, const uint64_t *__restrict__ k2, uint32_t nLines,
                                 uint32_t *__restrict__ hdrLine, uint32_t *__restrict__ seqSrc, uint32_t *__restrict__ seqDst)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nLines) return;
    const uint64_t a = k1[i];
    if (i == nLines) { hdrLine[(uint32_t)(a >> 32)] = nLines; seqDst[(uint32_t)a] = (uint32_t)(k2[i] >> 32); return; }
    const uint64_t b = k1[i + 1], p = k2[i];
    if ((b >> 32) != (a >> 32)) hdrLine[(uint32_t)(a >> 32)] = i;
    if ((uint32_t)b != (uint32_t)a && (k2[i + 1] >> 32) != (p >> 32)) { seqSrc[(uint32_t)a] = lineStart[i]; seqDst[(uint32_t)a] = (uint32_t)(p >> 32); }
}

// One lane per read (and one for the end): off, nameOff, lengths at the pool's end; the names' places for the gather.
__global__ void prs_reads_kernel(const uint32_t *__restrict__ lineStart, const uint32_t *__restrict__ hdrLine, const uint64_t *__restrict__ k1,
                                 const uint64_t *__restrict__ k2, uint32_t nReads, uint64_t longSeq, int64_t baseBase, uint64_t nameBase,
                                 int64_t *__restrict__ off, uint64_t *__restrict__ nameOff, uint32_t *__restrict__ lengths,
                                 uint32_t *__restrict__ nameSrc, uint32_t *__restrict__ nameDst, unsigned long long *__restrict__ status)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nReads) return;
    const uint32_t h = hdrLine[r];
    const uint64_t p = k2[h];
    off[r] = baseBase + (int64_t)(p >> 32);
    nameOff[r] = nameBase + (uint32_t)p;
    nameDst[r] = (uint32_t)p;
    if (r == nReads) return;
    const uint32_t h2 = hdrLine[r + 1];
    const uint64_t letters = (k2[h2] >> 32) - (p >> 32);
    lengths[r] = (uint32_t)letters + ((uint32_t)k1[h2] - (uint32_t)k1[h]);
    nameSrc[r] = lineStart[h] + 1;
    if (letters >= longSeq) atomicMin(status, status_key(lineStart[h], KASA_PARSE_LONG));
}

// largest j in [lo, hi] with dst[j] <= o (dst ascends strictly, dst[lo] <= o)
__device__ __forceinline__ uint32_t prs_find(const uint32_t *__restrict__ dst, uint32_t lo, uint32_t hi, uint32_t o)
{
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo + 1) >> 1); if (dst[mid] <= o) lo = mid; else hi = mid - 1; }
    return lo;
}

// Entry j = text[src[j] ...) goes to output bytes [dst[j], dst[j + 1]); GATHER_NAMES: its last byte is a space instead,
// GATHER_RECORDS: a line feed (the text has one there, or nothing: a last line without one).  n >= 1 entries
// of at least one byte, dst[n] = total.  `out` is the 16-byte aligned address at or below the pool's end and `lead` what lies
// between the two, so that every store of a whole vector is aligned whatever the pool holds.
enum { GATHER_BASES = 0, GATHER_NAMES = 1, GATHER_RECORDS = 2 };
template <int KIND>
__global__ __launch_bounds__(64 * WAVES) void prs_gather_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ src, const uint32_t *__restrict__ dst,
                                                                uint32_t n, uint32_t total, uint8_t *__restrict__ out, uint32_t lead,
                                                                unsigned long long *__restrict__ status)
{
    constexpr bool NAMES = KIND != GATHER_BASES;                                 // the entry's last byte is not the text's
    constexpr uint32_t LAST = KIND == GATHER_NAMES ? (uint32_t)' ' : (uint32_t)'\n';
    constexpr bool BLANKS = KIND == GATHER_BASES;                                // only the letters are checked for ' ' and '\t'
    const uint32_t tile = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint64_t vEnd = (uint64_t)lead + total, v0 = (uint64_t)tile * TILE_BYTES;
    if (v0 >= vEnd) return;
    const uint64_t v1 = v0 + TILE_BYTES < vEnd ? v0 + TILE_BYTES : vEnd;
    const uint32_t jLo = prs_find(dst, 0, n - 1, (uint32_t)((v0 > lead ? v0 : lead) - lead));
    const uint32_t jHi = prs_find(dst, jLo, n - 1, (uint32_t)(v1 - 1 - lead));
    for (int s = 0; s < STEPS; ++s) {
        const uint64_t va = v0 + (uint64_t)s * STEP_BYTES + lane * 16;
        const uint64_t vb = va + 16 < vEnd ? va + 16 : vEnd, vs = va > lead ? va : lead;
        if (vs >= vb) continue;
        const uint32_t oLo = (uint32_t)(vs - lead), oHi = (uint32_t)(vb - lead);
        uint32_t j = prs_find(dst, jLo, jHi, oLo);
        uint32_t d0 = dst[j], d1 = dst[j + 1], s0 = src[j];
        uint32_t w[4] = {0, 0, 0, 0};
        uint32_t blankAt = ~0u;                                                  // the chunk position of the first ' ' or '\t' this lane met
        const bool whole = oHi - oLo == 16;
        if (whole && (uint64_t)oLo + 16 + (NAMES ? 1 : 0) <= d1) {
            // 16 bytes of one line: five dwords from the 4-byte aligned address below (the text is padded), shifted into place
            const uint32_t a = s0 + (oLo - d0);
            const uint32_t *q = reinterpret_cast<const uint32_t *>(text + (a & ~3u));
            const uint32_t sh = a & 3u, x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3], x4 = q[4];
            w[0] = __builtin_amdgcn_alignbyte(x1, x0, sh); w[1] = __builtin_amdgcn_alignbyte(x2, x1, sh);
            w[2] = __builtin_amdgcn_alignbyte(x3, x2, sh); w[3] = __builtin_amdgcn_alignbyte(x4, x3, sh);
            if (BLANKS && (eq_bytes(w[0], 0x20202020u) | eq_bytes(w[1], 0x20202020u) | eq_bytes(w[2], 0x20202020u) | eq_bytes(w[3], 0x20202020u) |
                           eq_bytes(w[0], 0x09090909u) | eq_bytes(w[1], 0x09090909u) | eq_bytes(w[2], 0x09090909u) | eq_bytes(w[3], 0x09090909u)) != 0)
                for (int q = 15; q >= 0; --q) { const uint32_t c = (w[q >> 2] >> (8 * (q & 3))) & 0xFFu; if (c == ' ' || c == '\t') blankAt = a + q; }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const uint64_t v = va + q;
                if (v < vs || v >= vb) continue;
                const uint32_t k = (uint32_t)(v - lead);
                while (k >= d1) { ++j; d0 = d1; d1 = dst[j + 1]; s0 = src[j]; }       // (every entry has a byte: at most 16 steps per lane)
                const uint32_t c = (NAMES && k == d1 - 1) ? LAST : (uint32_t)text[s0 + (k - d0)];
                if (BLANKS && (c == ' ' || c == '\t') && blankAt == ~0u) blankAt = s0 + (k - d0);
                w[q >> 2] |= c << (8 * (q & 3));
            }
        }
        if (blankAt != ~0u) atomicMin(status, status_key(blankAt, KASA_PARSE_BLANK));
        if (whole) *reinterpret_cast<uint4 *>(out + va) = make_uint4(w[0], w[1], w[2], w[3]);
        else
            for (int q = 0; q < 16; ++q) { const uint64_t v = va + q; if (v >= vs && v < vb) out[v] = (uint8_t)(w[q >> 2] >> (8 * (q & 3))); }
    }
}

// ---- the records (kasa_pool_keep_records).  k3 = non-empty lines << 32 | their bytes with one line feed each (a chunk and
// one added line feed stay below 2^32); entry nLines = 0: the running sum's totals land there.
__global__ void prs_recsize_kernel(const uint32_t *__restrict__ lineStart, uint32_t nLines, uint64_t *__restrict__ k3)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nLines) return;
    const uint32_t len = i < nLines ? lineStart[i + 1] - 1 - lineStart[i] : 0;
    k3[i] = len ? (1ull << 32) | (uint64_t)(len + 1) : 0;
}
// after the running sum: the non-empty lines in order with their place in the records' text
__global__ void prs_recindex_kernel(const uint32_t *__restrict__ lineStart, const uint64_t *__restrict__ k3, uint32_t nLines, uint32_t *__restrict__ recSrc, uint32_t *__restrict__ recDst)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nLines) return;
    const uint64_t a = k3[i];
    if (i == nLines) { recDst[(uint32_t)(a >> 32)] = (uint32_t)a; return; }
    if ((k3[i + 1] >> 32) != (a >> 32)) { recSrc[(uint32_t)(a >> 32)] = lineStart[i]; recDst[(uint32_t)(a >> 32)] = (uint32_t)a; }
}
// one lane per read and one for the end: a record starts with its header line
__global__ void prs_recoff_kernel(const uint32_t *__restrict__ hdrLine, const uint64_t *__restrict__ k3, uint32_t nReads, uint64_t recBase, uint64_t *__restrict__ recOff)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= nReads) recOff[r] = recBase + (uint32_t)k3[hdrLine[r]];
}

// the FASTA cut of kasa_bgzf_parse_append: the last line that begins with '>' as line << 32 | its start (the key grows with the line)
__global__ void prs_last_header_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ lineStart, uint32_t nLines, uint32_t nBytes, unsigned long long *__restrict__ last)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nLines) return;
    const uint32_t s = lineStart[i];
    if (s < nBytes && text[s] == '>') atomicMax(last, ((unsigned long long)i << 32) | s);
}

// the reads a take left behind move to the front of the pool's other set of arrays
template <class T> __global__ void prs_rebase_kernel(const T *__restrict__ src, T *__restrict__ dst, uint64_t n, T delta)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i] - delta;
}

// the ends of reads [r0, r0 + n) in letters and name bytes: four values for ONE read-back
__global__ void prs_ends_kernel(const int64_t *__restrict__ off, const uint64_t *__restrict__ nameOff, uint64_t r0, uint64_t n, uint64_t *__restrict__ out)
{
    out[0] = (uint64_t)off[r0]; out[1] = (uint64_t)off[r0 + n]; out[2] = nameOff[r0]; out[3] = nameOff[r0 + n];
}

// ---- pairs: two pools read as ONE run of mate-interleaved entries (kasa_pair_take, kasa_pair_fetch) ----
// Entry j of 2n is mate j & 1 of pair j >> 1.  With a, b the two pools' running offsets from the first pair on and a0, b0
// their values there, entry j starts at output byte
//   D(j) = (a[(j >> 1) + (j & 1)] - a0) + (b[j >> 1] - b0),        D(2n) = total,
// and its bytes lie at src1 + a[j >> 1] (mate 1) or src2 + b[j >> 1] (mate 2): no scan and no table of entries.  Letters
// (off) and names (nameOff) are laid out alike, so one gather serves both.  An entry may be EMPTY (a FASTA record without
// sequence lines): D ascends, but not strictly.
struct PairOffsets {
    const uint64_t *a, *b;
    uint64_t a0, b0;
    __device__ __forceinline__ uint64_t dst(uint64_t j) const { return (a[(j >> 1) + (j & 1)] - a0) + (b[j >> 1] - b0); }
    __device__ __forceinline__ uint64_t src(uint64_t j) const { return (j & 1) ? b[j >> 1] : a[j >> 1]; }
    __device__ __forceinline__ const uint8_t *base(uint64_t j, const uint8_t *src1, const uint8_t *src2) const { return (j & 1) ? src2 : src1; }
    // largest j in [lo, hi] with D(j) <= o; for o < D(hi + 1) that entry holds byte o: the empty ones before it are stepped over
    __device__ __forceinline__ uint64_t find(uint64_t lo, uint64_t hi, uint64_t o) const
    {
        while (lo < hi) { const uint64_t mid = lo + ((hi - lo + 1) >> 1); if (dst(mid) <= o) lo = mid; else hi = mid - 1; }
        return lo;
    }
};

// one lane per pair and one for the end; every output may be NULL.  lo: the letters' offsets, na: the names'.
__global__ void pair_layout_kernel(PairOffsets lo, PairOffsets na, const uint32_t *__restrict__ len1, const uint32_t *__restrict__ len2, uint64_t n,
                                   int64_t *__restrict__ off, uint32_t *__restrict__ seqRead, uint64_t *__restrict__ nameOff, uint32_t *__restrict__ lengths)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n) return;
    if (off) {
        const uint64_t y = lo.b[r] - lo.b0;
        off[2 * r] = (int64_t)((lo.a[r] - lo.a0) + y);
        if (r < n) off[2 * r + 1] = (int64_t)((lo.a[r + 1] - lo.a0) + y);
    }
    if (nameOff) nameOff[r] = (na.a[r] - na.a0) + (na.b[r] - na.b0);
    if (r == n) return;
    if (seqRead) { seqRead[2 * r] = (uint32_t)r; seqRead[2 * r + 1] = (uint32_t)r; }
    if (lengths) lengths[r] = len1[r] + len2[r];
}

// The copy, split by OUTPUT bytes like prs_gather_kernel: a wavefront owns TILE_BYTES of `out` (16-byte aligned), finds the
// entries of its tile by bisection in D, every lane the entry of its 16 bytes.  16 bytes of one entry: five dwords from the
// 4-byte aligned address below (both sources are padded behind their end, pool_room), shifted into place, one aligned store.
// Lanes whose 16 bytes cross a junction, and the tail, go byte by byte.  nEntries >= 1, total >= 1; positions are 64-bit.
// Offsets names the entries: dst(j) (ascending, dst(nEntries) = total), src(j), base(j, src1, src2), find -- PairOffsets above
// (2 n entries of two pools), kasa_filter's FilterOffsets (the reads of one side of --filter, one source).
template <class Offsets>
__global__ __launch_bounds__(64 * WAVES) void pair_gather_kernel(const uint8_t *__restrict__ src1, const uint8_t *__restrict__ src2, Offsets d, uint64_t nEntries,
                                                                 uint64_t total, uint8_t *__restrict__ out)
{
    const uint64_t tile = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t v0 = tile * TILE_BYTES;
    if (v0 >= total) return;
    const uint64_t v1 = v0 + TILE_BYTES < total ? v0 + TILE_BYTES : total;
    const uint64_t jLo = d.find(0, nEntries - 1, v0), jHi = d.find(jLo, nEntries - 1, v1 - 1);
    for (int s = 0; s < STEPS; ++s) {
        const uint64_t va = v0 + (uint64_t)s * STEP_BYTES + lane * 16;
        if (va >= total) continue;
        const uint64_t vb = va + 16 < total ? va + 16 : total;
        uint64_t j = d.find(jLo, jHi, va);
        uint64_t d0 = d.dst(j), d1 = d.dst(j + 1);
        const uint8_t *sp = d.base(j, src1, src2) + d.src(j);
        uint32_t w[4] = {0, 0, 0, 0};
        const bool whole = vb - va == 16;
        if (whole && va + 16 <= d1) {
            const uint8_t *p = sp + (va - d0);
            const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
            const uint32_t *q = reinterpret_cast<const uint32_t *>(p - sh);
            const uint32_t x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3], x4 = q[4];
            w[0] = __builtin_amdgcn_alignbyte(x1, x0, sh); w[1] = __builtin_amdgcn_alignbyte(x2, x1, sh);
            w[2] = __builtin_amdgcn_alignbyte(x3, x2, sh); w[3] = __builtin_amdgcn_alignbyte(x4, x3, sh);
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const uint64_t k = va + q;
                if (k >= vb) continue;
                while (k >= d1) { ++j; d0 = d1; d1 = d.dst(j + 1); sp = d.base(j, src1, src2) + d.src(j); }   // (k < total = dst(nEntries): it ends; empty entries fall through)
                w[q >> 2] |= (uint32_t)sp[k - d0] << (8 * (q & 3));
            }
        }
        if (whole) *reinterpret_cast<uint4 *>(out + va) = make_uint4(w[0], w[1], w[2], w[3]);
        else
#pragma unroll
            for (int q = 0; q < 16; ++q) { const uint64_t k = va + q; if (k < vb) out[k] = (uint8_t)(w[q >> 2] >> (8 * (q & 3))); }
    }
}

struct PoolArrays { DevBuf bases, off, names, nameOff, lengths, records, recOff; };   // the last two with kasa_pool_keep_records only

}  // namespace kasa_parse_impl

struct kasa_parser {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    uint64_t longSeq = 0;
    // reads [head, nReads) of arrays[cur] are the pool: off / nameOff keep running values, a fetch or take rebases them
    kasa_parse_impl::PoolArrays arrays[2];
    int cur = 0;
    uint64_t head = 0, nReads = 0, headBase = 0, endBase = 0, headName = 0, endName = 0;
    DevBuf text, tileCnt, lineStart, k1, k2, hdrLine, seqSrc, seqDst, nameSrc, nameDst, scanTmp, status;
    int lastCode = 0; uint64_t lastAt = 0;
    double msUpload = 0, msParse = 0;
    // kasa_bgzf_parse_append: the text behind the last whole record stays at the front of `text` for the next span
    uint64_t carry = 0;
    DevBuf zStream, zTab, carryTmp;
    hipEvent_t evz[2] = {nullptr, nullptr};
    int inflateCode = 0; uint64_t inflateMember = 0;
    double msInflate = 0;
    // kasa_gzip_parse_append: where the one long stream stands between two spans -- what comes next at the span's first byte
    // (a member header, deflate data from bit `bit` on, a trailer), the member's CRC-32 register and length so far, and the
    // last winLen bytes of its text at the end of gzWin's 32 KiB
    struct GzState { int phase = 0; uint32_t bit = 0, crcReg = 0, winLen = 0; uint64_t memberBytes = 0, member = 0; } gz;
    DevBuf gzWin, gzTmp;
    uint64_t gzStats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // kasa_pair_fetch (this pool as the first of the two): the interleaved arrays before they cross to the host
    DevBuf pairOff, pairNameOff, pairLengths, pairNames, pairBases;
    // kasa_pool_keep_records: records / recOff of the pool's arrays are kept like names / nameOff
    bool keepRecords = false;
    uint64_t headRec = 0, endRec = 0;
    DevBuf k3, recSrc, recDst;
};

namespace kasa_parse_impl {

static int grow_keep(DevBuf &b, size_t need, size_t keep, hipStream_t stream)
{
    if (need <= b.cap) return KASA_OK;
    DevBuf nb;
    int rc = nb.reserve(std::max(need, b.cap + b.cap / 2));
    if (rc) return rc;
    if (keep) HIPCHK(hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    b = std::move(nb);
    return KASA_OK;
}

// room for `addReads` reads of `addBases` letters and `addNames` name bytes behind what set `a` holds (kept)
static int pool_room(kasa_parser *p, PoolArrays &a, uint64_t reads, uint64_t bases, uint64_t names, uint64_t addReads, uint64_t addBases, uint64_t addNames, bool fresh)
{
    int rc;
    if ((rc = grow_keep(a.bases, bases + addBases + 64, fresh ? 0 : bases, p->stream)) || (rc = grow_keep(a.names, names + addNames + 64, fresh ? 0 : names, p->stream)) ||
        (rc = grow_keep(a.off, (reads + addReads + 1) * 8, fresh ? 0 : (reads + 1) * 8, p->stream)) ||
        (rc = grow_keep(a.nameOff, (reads + addReads + 1) * 8, fresh ? 0 : (reads + 1) * 8, p->stream)) ||
        (rc = grow_keep(a.lengths, (reads + addReads) * 4 + 64, fresh ? 0 : reads * 4, p->stream)))
        return rc;
    return KASA_OK;
}
// ... and of `addRecs` bytes of record text behind `recs` (the 64 bytes of slack: the gathers' five-dword reads end behind a record)
static int pool_room_records(kasa_parser *p, PoolArrays &a, uint64_t reads, uint64_t recs, uint64_t addReads, uint64_t addRecs, bool fresh)
{
    int rc;
    if ((rc = grow_keep(a.records, recs + addRecs + 64, fresh ? 0 : recs, p->stream)) ||
        (rc = grow_keep(a.recOff, (reads + addReads + 1) * 8, fresh ? 0 : (reads + 1) * 8, p->stream)))
        return rc;
    return KASA_OK;
}

// The reads already taken leave the arrays.  An empty pool starts over where it is (off[0] = nameOff[0] = 0 again, nothing
// copied); a remainder moves to the front of the other set once the taken letters outweigh it, so that the copies stay
// below the bytes appended and the arrays below twice the pool plus a chunk.
static int pool_compact(kasa_parser *p)
{
    if (p->head == 0) return KASA_OK;
    const uint64_t n = p->nReads - p->head, nb = p->endBase - p->headBase, nn = p->endName - p->headName;
    if (n == 0) {
        HIPCHK(hipMemsetAsync(p->arrays[p->cur].off.p, 0, 8, p->stream));
        HIPCHK(hipMemsetAsync(p->arrays[p->cur].nameOff.p, 0, 8, p->stream));
        if (p->keepRecords) HIPCHK(hipMemsetAsync(p->arrays[p->cur].recOff.p, 0, 8, p->stream));
        p->head = p->nReads = 0; p->headBase = p->endBase = 0; p->headName = p->endName = 0; p->headRec = p->endRec = 0;
        return KASA_OK;
    }
    if (p->headBase <= nb) return KASA_OK;
    PoolArrays &from = p->arrays[p->cur], &to = p->arrays[p->cur ^ 1];
    const uint64_t nr = p->endRec - p->headRec;
    int rc = pool_room(p, to, 0, 0, 0, n, nb, nn, true);
    if (rc) return rc;
    if (p->keepRecords) {
        if ((rc = pool_room_records(p, to, 0, 0, n, nr, true))) return rc;
        if (nr) HIPCHK(hipMemcpyAsync(to.records.p, from.records.as<char>() + p->headRec, nr, hipMemcpyDeviceToDevice, p->stream));
        prs_rebase_kernel<uint64_t><<<blocks_for(n + 1, 256), 256, 0, p->stream>>>(from.recOff.as<uint64_t>() + p->head, to.recOff.as<uint64_t>(), n + 1, p->headRec);
    }
    if (nb) HIPCHK(hipMemcpyAsync(to.bases.p, from.bases.as<uint8_t>() + p->headBase, nb, hipMemcpyDeviceToDevice, p->stream));
    if (nn) HIPCHK(hipMemcpyAsync(to.names.p, from.names.as<char>() + p->headName, nn, hipMemcpyDeviceToDevice, p->stream));
    if (n) HIPCHK(hipMemcpyAsync(to.lengths.p, from.lengths.as<uint32_t>() + p->head, n * 4, hipMemcpyDeviceToDevice, p->stream));
    prs_rebase_kernel<int64_t><<<blocks_for(n + 1, 256), 256, 0, p->stream>>>(from.off.as<int64_t>() + p->head, to.off.as<int64_t>(), n + 1, (int64_t)p->headBase);
    prs_rebase_kernel<uint64_t><<<blocks_for(n + 1, 256), 256, 0, p->stream>>>(from.nameOff.as<uint64_t>() + p->head, to.nameOff.as<uint64_t>(), n + 1, p->headName);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(p->stream));
    p->cur ^= 1; p->head = 0; p->nReads = n; p->headBase = 0; p->endBase = nb; p->headName = 0; p->endName = nn; p->headRec = 0; p->endRec = nr;
    return KASA_OK;
}

static int refuse(kasa_parser *p, int code, uint64_t at, int *parsable)
{
    p->lastCode = code; p->lastAt = at;
    if (parsable) *parsable = 0;
    return KASA_OK;
}

// How the text that is on the device is cut before it is parsed (kasa_bgzf_parse_append; `cut` = nullptr: all of it, and its
// first and last byte are known on the host).
struct TextCut {
    bool final = false;
    uint64_t cutBytes = 0;                        // out: the text up to here was parsed (0 with *parsable = 0)
};

static int append_device(kasa_parser *p, uint64_t nBytes, int firstByte, int lastByte, int fasta, TextCut *cut, uint64_t *nReadsAdded, int *parsable);

static int append_impl(kasa_parser *p, const char *text, uint64_t nBytes, int fasta, uint64_t *nReadsAdded, int *parsable)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (nBytes && !text) return fail(KASA_E_ARG, "kasa_parse_append: text is NULL");
    if (p->carry) return fail(KASA_E_STATE, "kasa_parse_append: %llu bytes of a BGZF span are carried (kasa_bgzf_parse_append with final set takes them)", (unsigned long long)p->carry);
    if (nReadsAdded) *nReadsAdded = 0;
    if (parsable) *parsable = 1;
    p->lastCode = KASA_PARSE_OK; p->lastAt = 0;
    if (nBytes == 0) return KASA_OK;
    if (nBytes >= MAX_CHUNK) return refuse(p, KASA_PARSE_TOO_LARGE, 0, parsable);
    if (fasta && text[0] != '>') return refuse(p, KASA_PARSE_FASTA_HEADER, 0, parsable);
    HIPCHK(hipSetDevice(p->device));
    int rc;
    if ((rc = pool_compact(p))) return rc;
    const uint32_t nTiles = (uint32_t)((nBytes + TILE_BYTES - 1) / TILE_BYTES);
    const size_t padded = (size_t)nTiles * TILE_BYTES + 64;
    if ((rc = p->text.reserve(padded))) return rc;
    HIPCHK(hipEventRecord(p->ev[0], p->stream));
    HIPCHK(hipMemcpyAsync(p->text.p, text, nBytes, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemsetAsync(p->text.as<uint8_t>() + nBytes, 0, padded - nBytes, p->stream));
    HIPCHK(hipEventRecord(p->ev[1], p->stream));
    return append_device(p, nBytes, (unsigned char)text[0], (unsigned char)text[nBytes - 1], fasta, nullptr, nReadsAdded, parsable);
}

// The text is in p->text (nBytes of it, zeros behind up to a whole tile + 64; ev[0] .. ev[1] spans how it got there).
static int append_device(kasa_parser *p, uint64_t nBytes, int firstByte, int lastByte, int fasta, TextCut *cut, uint64_t *nReadsAdded, int *parsable)
{
    int rc;
    const uint32_t nTiles = (uint32_t)((nBytes + TILE_BYTES - 1) / TILE_BYTES);
    if ((rc = p->tileCnt.reserve(((size_t)nTiles + 1) * 4)) || (rc = p->status.reserve(64))) return rc;
    HIPCHK(hipMemsetAsync(p->status.p, 0xFF, 8, p->stream));
    // ---- line table
    uint32_t *tileCnt = p->tileCnt.as<uint32_t>();
    prs_count_kernel<<<blocks_for(nTiles, WAVES), 64 * WAVES, 0, p->stream>>>(p->text.as<uint4>(), nTiles, tileCnt);
    HIPCHK(hipGetLastError());
    if ((rc = dev_exclusive_scan(p->scanTmp, p->stream, tileCnt, tileCnt, 0u, (size_t)nTiles + 1, rocprim::plus<uint32_t>()))) return rc;
    uint32_t nFeeds = 0;
    uint8_t ends[2] = {(uint8_t)firstByte, (uint8_t)lastByte};
    if ((rc = fetch_async(p->stream, nFeeds, tileCnt + nTiles))) return rc;
    if (cut && ((rc = fetch_async(p->stream, ends[0], p->text.as<uint8_t>())) || (rc = fetch_async(p->stream, ends[1], p->text.as<uint8_t>() + nBytes - 1)))) return rc;   // (nobody on the host has seen this text)
    HIPCHK(hipStreamSynchronize(p->stream));
    int trailingFeed = ends[1] == '\n';
    uint32_t nLines = nFeeds + (trailingFeed ? 0u : 1u);                               // of the whole text: the line table covers all of it
    const size_t nl = (size_t)nLines + 2;
    if ((rc = p->lineStart.reserve(nl * 4)) || (rc = p->k1.reserve(nl * 8)) || (rc = p->k2.reserve(nl * 8)) || (rc = p->hdrLine.reserve(nl * 4)) ||
        (rc = p->seqSrc.reserve(nl * 4)) || (rc = p->seqDst.reserve(nl * 4)))
        return rc;
    uint32_t *lineStart = p->lineStart.as<uint32_t>();
    uint64_t *k1 = p->k1.as<uint64_t>(), *k2 = p->k2.as<uint64_t>();
    unsigned long long *status = p->status.as<unsigned long long>();
    prs_lines_kernel<<<blocks_for(nTiles, WAVES), 64 * WAVES, 0, p->stream>>>(p->text.as<uint4>(), nTiles, tileCnt, lineStart, nLines, (uint32_t)nBytes, trailingFeed);
    HIPCHK(hipGetLastError());
    if (cut && fasta && ends[0] != '>') return refuse(p, KASA_PARSE_FASTA_HEADER, 0, parsable);   // (before anything is carried: as kasa_parse_append refuses it)
    if (cut && !cut->final) {
        // ---- the cut, from the same line table: the parse sees lines [0, nLines) = text [0, cutBytes), which ends with a line feed
        uint32_t useLines = 0, cutAt = 0;
        if (!fasta) {                                                                // the last line feed that closes a fourth line
            useLines = nFeeds & ~3u;
            if (useLines && (rc = fetch_async(p->stream, cutAt, lineStart + useLines))) return rc;
            HIPCHK(hipStreamSynchronize(p->stream));
        } else {                                                                     // the start of the last line that begins with '>'
            unsigned long long *last = status + 1, key = 0;                          // (behind the status word)
            HIPCHK(hipMemsetAsync(last, 0, 8, p->stream));
            prs_last_header_kernel<<<blocks_for(nLines, 256), 256, 0, p->stream>>>(p->text.as<uint8_t>(), lineStart, nLines, (uint32_t)nBytes, last);
            HIPCHK(hipGetLastError());
            if ((rc = fetch(p->stream, key, last))) return rc;
            useLines = (uint32_t)(key >> 32); cutAt = (uint32_t)key;
        }
        if (useLines == 0 || cutAt == 0) return KASA_OK;                             // no whole record yet: everything is carried
        nLines = useLines; nBytes = cutAt; trailingFeed = 1;
    }
    if (cut) cut->cutBytes = nBytes;
    // ---- classify
    prs_classify_kernel<<<blocks_for((uint64_t)nLines + 1, 256), 256, 0, p->stream>>>(p->text.as<uint8_t>(), lineStart, nLines, fasta, p->longSeq, k1, k2, status);
    HIPCHK(hipGetLastError());
    if ((rc = dev_exclusive_scan(p->scanTmp, p->stream, k1, k1, (uint64_t)0, (size_t)nLines + 1, rocprim::plus<uint64_t>())) ||
        (rc = dev_exclusive_scan(p->scanTmp, p->stream, k2, k2, (uint64_t)0, (size_t)nLines + 1, rocprim::plus<uint64_t>()))) return rc;
    prs_index_kernel<<<blocks_for((uint64_t)nLines + 1, 256), 256, 0, p->stream>>>(lineStart, k1, k2, nLines, p->hdrLine.as<uint32_t>(), p->seqSrc.as<uint32_t>(), p->seqDst.as<uint32_t>());
    HIPCHK(hipGetLastError());
    uint64_t tot[2] = {0, 0}, totRec = 0;
    unsigned long long st = ~0ull;
    if (p->keepRecords) {                                                          // ---- the records' sizes: one more running sum over the lines
        if ((rc = p->k3.reserve(nl * 8)) || (rc = p->recSrc.reserve(nl * 4)) || (rc = p->recDst.reserve(nl * 4))) return rc;
        uint64_t *k3 = p->k3.as<uint64_t>();
        prs_recsize_kernel<<<blocks_for((uint64_t)nLines + 1, 256), 256, 0, p->stream>>>(lineStart, nLines, k3);
        HIPCHK(hipGetLastError());
        if ((rc = dev_exclusive_scan(p->scanTmp, p->stream, k3, k3, (uint64_t)0, (size_t)nLines + 1, rocprim::plus<uint64_t>()))) return rc;
        prs_recindex_kernel<<<blocks_for((uint64_t)nLines + 1, 256), 256, 0, p->stream>>>(lineStart, k3, nLines, p->recSrc.as<uint32_t>(), p->recDst.as<uint32_t>());
        HIPCHK(hipGetLastError());
        if ((rc = fetch_async(p->stream, totRec, k3 + nLines))) return rc;
    }
    if ((rc = fetch_async(p->stream, tot[0], k1 + nLines)) || (rc = fetch_async(p->stream, tot[1], k2 + nLines)) || (rc = fetch(p->stream, st, status))) return rc;
    if (st != ~0ull) {                                                             // (the text went up all the same: it counts)
        float up = 0.0f;
        if (!cut && hipEventElapsedTime(&up, p->ev[0], p->ev[1]) == hipSuccess) p->msUpload += up;
        return refuse(p, (int)(st & 0xFF), st >> 8, parsable);
    }
    const uint64_t addReads = tot[0] >> 32, addBases = tot[1] >> 32, addNames = tot[1] & 0xFFFFFFFFull;
    // FASTA sequence lines counted = the non-empty ones = the gather's entries; FASTQ: one per read, none empty
    const uint32_t nSeqLines = (uint32_t)tot[0];
    PoolArrays &a = p->arrays[p->cur];
    if ((rc = pool_room(p, a, p->nReads, p->endBase, p->endName, addReads, addBases, addNames, false)) ||
        (rc = p->nameSrc.reserve((addReads + 2) * 4)) || (rc = p->nameDst.reserve((addReads + 2) * 4)))
        return rc;
    const uint32_t nRecLines = (uint32_t)(totRec >> 32);
    const uint64_t addRecs = totRec & 0xFFFFFFFFull;
    if (p->keepRecords && (rc = pool_room_records(p, a, p->nReads, p->endRec, addReads, addRecs, false))) return rc;
    // ---- per read, then the two gathers behind the pool's end
    prs_reads_kernel<<<blocks_for(addReads + 1, 256), 256, 0, p->stream>>>(lineStart, p->hdrLine.as<uint32_t>(), k1, k2, (uint32_t)addReads, p->longSeq,
        (int64_t)p->endBase, p->endName, a.off.as<int64_t>() + p->nReads, a.nameOff.as<uint64_t>() + p->nReads, a.lengths.as<uint32_t>() + p->nReads,
        p->nameSrc.as<uint32_t>(), p->nameDst.as<uint32_t>(), status);
    HIPCHK(hipGetLastError());
    if (addBases && nSeqLines) {
        const uint32_t lead = (uint32_t)(p->endBase & 15);
        const uint64_t tiles = (lead + addBases + TILE_BYTES - 1) / TILE_BYTES;
        prs_gather_kernel<GATHER_BASES><<<blocks_for(tiles, WAVES), 64 * WAVES, 0, p->stream>>>(p->text.as<uint8_t>(), p->seqSrc.as<uint32_t>(), p->seqDst.as<uint32_t>(),
            nSeqLines, (uint32_t)addBases, a.bases.as<uint8_t>() + (p->endBase - lead), lead, status);
        HIPCHK(hipGetLastError());
    }
    if (addNames && addReads) {
        const uint32_t lead = (uint32_t)(p->endName & 15);
        const uint64_t tiles = (lead + addNames + TILE_BYTES - 1) / TILE_BYTES;
        prs_gather_kernel<GATHER_NAMES><<<blocks_for(tiles, WAVES), 64 * WAVES, 0, p->stream>>>(p->text.as<uint8_t>(), p->nameSrc.as<uint32_t>(), p->nameDst.as<uint32_t>(),
            (uint32_t)addReads, (uint32_t)addNames, a.names.as<uint8_t>() + (p->endName - lead), lead, status);
        HIPCHK(hipGetLastError());
    }
    if (p->keepRecords) {
        prs_recoff_kernel<<<blocks_for(addReads + 1, 256), 256, 0, p->stream>>>(p->hdrLine.as<uint32_t>(), p->k3.as<uint64_t>(), (uint32_t)addReads, p->endRec,
            a.recOff.as<uint64_t>() + p->nReads);
        HIPCHK(hipGetLastError());
        if (addRecs && nRecLines) {
            const uint32_t lead = (uint32_t)(p->endRec & 15);
            const uint64_t tiles = (lead + addRecs + TILE_BYTES - 1) / TILE_BYTES;
            prs_gather_kernel<GATHER_RECORDS><<<blocks_for(tiles, WAVES), 64 * WAVES, 0, p->stream>>>(p->text.as<uint8_t>(), p->recSrc.as<uint32_t>(), p->recDst.as<uint32_t>(),
                nRecLines, (uint32_t)addRecs, a.records.as<uint8_t>() + (p->endRec - lead), lead, status);
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipEventRecord(p->ev[2], p->stream));
    if ((rc = fetch(p->stream, st, status))) return rc;
    float ms = 0.0f;
    if (!cut && hipEventElapsedTime(&ms, p->ev[0], p->ev[1]) == hipSuccess) p->msUpload += ms;       // (a span's upload and inflate are counted where they happen)
    if (hipEventElapsedTime(&ms, cut ? p->evz[1] : p->ev[1], p->ev[2]) == hipSuccess) p->msParse += ms;
    if (st != ~0ull) return refuse(p, (int)(st & 0xFF), st >> 8, parsable);         // (what was written lies behind the pool's end)
    p->nReads += addReads; p->endBase += addBases; p->endName += addNames; p->endRec += addRecs;
    if (nReadsAdded) *nReadsAdded = addReads;
    return KASA_OK;
}

// A span of whole BGZF members: inflated behind the carry, cut at the last whole record, parsed; what lies behind the cut is
// the next carry.  Nothing changes -- pool, carry -- unless the span inflates cleanly and the cut text parses.
static int append_bgzf_impl(kasa_parser *p, const uint8_t *span, uint64_t nBytes, int fasta, int final, uint64_t *nReadsAdded, int *parsable,
                            uint64_t *nTextBytes, uint64_t *carryBytes)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (nBytes && !span) return fail(KASA_E_ARG, "kasa_bgzf_parse_append: members is NULL");
    if (nReadsAdded) *nReadsAdded = 0;
    if (parsable) *parsable = 1;
    if (nTextBytes) *nTextBytes = 0;
    if (carryBytes) *carryBytes = p->carry;
    p->lastCode = KASA_PARSE_OK; p->lastAt = 0; p->inflateCode = KASA_INFLATE_OK; p->inflateMember = 0;
    std::vector<kasa_inflate::Member> tab;
    uint64_t consumed = 0, nText = 0;
    int zs = kasa_inflate::walk_members(span, nBytes, tab, &consumed, &nText);
    if (zs == KASA_INFLATE_OK && consumed != nBytes) zs = KASA_INFLATE_CUT;
    if (zs != KASA_INFLATE_OK) { p->inflateCode = zs; p->inflateMember = tab.size(); return refuse(p, KASA_PARSE_INFLATE, tab.size(), parsable); }
    if (tab.size() > 0x7FFFFFFFull) return fail(KASA_E_LIMIT, "kasa_bgzf_parse_append: %zu members are more than one call takes", tab.size());
    const uint64_t total = p->carry + nText;
    if (total >= MAX_CHUNK) return refuse(p, KASA_PARSE_TOO_LARGE, 0, parsable);
    if (total == 0) return KASA_OK;
    HIPCHK(hipSetDevice(p->device));
    int rc;
    if ((rc = pool_compact(p))) return rc;
    const uint32_t nTiles = (uint32_t)((total + TILE_BYTES - 1) / TILE_BYTES);
    const size_t padded = (size_t)nTiles * TILE_BYTES + 64;
    if ((rc = grow_keep(p->text, padded, p->carry, p->stream)) || (rc = p->status.reserve(64))) return rc;
    uint8_t *text = p->text.as<uint8_t>();
    HIPCHK(hipEventRecord(p->ev[0], p->stream));
    HIPCHK(hipEventRecord(p->evz[0], p->stream));
    if (!tab.empty() && nText) {
        if ((rc = p->zStream.reserve(nBytes)) || (rc = p->zTab.reserve(tab.size() * sizeof(kasa_inflate::Member)))) return rc;
        HIPCHK(hipMemcpyAsync(p->zStream.p, span, nBytes, hipMemcpyHostToDevice, p->stream));
        HIPCHK(hipMemcpyAsync(p->zTab.p, tab.data(), tab.size() * sizeof(kasa_inflate::Member), hipMemcpyHostToDevice, p->stream));
        HIPCHK(hipMemsetAsync(p->status.p, 0xFF, 8, p->stream));
        HIPCHK(hipEventRecord(p->evz[0], p->stream));
        kasa_inflate::inflate_kernel<<<(uint32_t)tab.size(), 64, 0, p->stream>>>(p->zStream.as<uint8_t>(), p->zTab.as<kasa_inflate::Member>(), (uint32_t)tab.size(),
                                                                                text + p->carry, p->status.as<unsigned long long>());
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemsetAsync(text + total, 0, padded - total, p->stream));
    HIPCHK(hipEventRecord(p->evz[1], p->stream));
    unsigned long long st = ~0ull;
    if (!tab.empty() && nText && (rc = fetch_async(p->stream, st, p->status.as<unsigned long long>()))) return rc;
    HIPCHK(hipStreamSynchronize(p->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, p->ev[0], p->evz[0]) == hipSuccess) p->msUpload += ms;
    if (hipEventElapsedTime(&ms, p->evz[0], p->evz[1]) == hipSuccess) p->msInflate += ms;
    if (st != ~0ull) { p->inflateCode = (int)(st & 0xFF); p->inflateMember = st >> 8; return refuse(p, KASA_PARSE_INFLATE, st >> 8, parsable); }
    TextCut cut;
    cut.final = final != 0;
    int ok = 1;
    uint64_t added = 0;
    if ((rc = append_device(p, total, 0, 0, fasta, &cut, &added, &ok))) return rc;
    if (!ok) { if (parsable) *parsable = 0; return KASA_OK; }                      // (the carry is where it was; the text behind it is given up)
    // ---- what lies behind the cut moves to the front
    const uint64_t rest = total - cut.cutBytes;
    if (rest && cut.cutBytes) {
        if (rest <= cut.cutBytes) HIPCHK(hipMemcpyAsync(text, text + cut.cutBytes, rest, hipMemcpyDeviceToDevice, p->stream));
        else {                                                                      // (the two ranges overlap: by way of a buffer)
            if ((rc = p->carryTmp.reserve(rest))) return rc;
            HIPCHK(hipMemcpyAsync(p->carryTmp.p, text + cut.cutBytes, rest, hipMemcpyDeviceToDevice, p->stream));
            HIPCHK(hipMemcpyAsync(text, p->carryTmp.p, rest, hipMemcpyDeviceToDevice, p->stream));
        }
        HIPCHK(hipStreamSynchronize(p->stream));
    }
    p->carry = rest;
    if (nReadsAdded) *nReadsAdded = added;
    if (nTextBytes) *nTextBytes = cut.cutBytes;
    if (carryBytes) *carryBytes = rest;
    return KASA_OK;
}

// The backend of kasa_gunzip.h's rounds whose destination is the parser's text behind the carry: it grows as the streams of the
// span are placed (their sizes are known only then).
struct GunzipIntoParser : GunzipDevice {
    kasa_parser *p = nullptr;
    uint64_t base = 0;                            // the carry: the span's text begins behind it
    int place(const std::vector<kasa_gunzip::Seg> &sg, uint64_t textAt, uint64_t total, uint64_t *markers, bool *bad)
    {
        const uint64_t end = base + textAt + total;
        if (end >= MAX_CHUNK) return fail(KASA_E_LIMIT, "kasa_gzip_parse_append: the span's text passes %llu bytes", (unsigned long long)MAX_CHUNK);
        int rc = grow_keep(p->text, (size_t)((end + TILE_BYTES - 1) / TILE_BYTES) * TILE_BYTES + 64, (size_t)(base + textAt), p->stream);
        if (rc) return rc;
        dText = p->text.as<uint8_t>() + base; textCap = textAt + total;
        return GunzipDevice::place(sg, textAt, total, markers, bad);
    }
};

// A span of a plain gzip file's bytes, from where the call before said (*keepFrom).  Whole blocks are inflated behind the carry
// (kasa_gunzip.h), the text is cut at the last whole record and parsed as append_bgzf_impl does.  Nothing changes -- pool,
// carry, the stream's state -- unless the span inflates cleanly and the cut text parses.
static int append_gzip_impl(kasa_parser *p, const uint8_t *span, uint64_t nBytes, int fasta, int final, uint64_t *nReadsAdded, int *parsable,
                            uint64_t *nTextBytes, uint64_t *keepFrom)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (nBytes && !span) return fail(KASA_E_ARG, "kasa_gzip_parse_append: bytes is NULL");
    if (nBytes >= (1ull << 31)) return fail(KASA_E_LIMIT, "kasa_gzip_parse_append: a span of %llu bytes is more than one call takes", (unsigned long long)nBytes);
    if (nReadsAdded) *nReadsAdded = 0;
    if (parsable) *parsable = 1;
    if (nTextBytes) *nTextBytes = 0;
    if (keepFrom) *keepFrom = 0;
    p->lastCode = KASA_PARSE_OK; p->lastAt = 0; p->inflateCode = KASA_INFLATE_OK; p->inflateMember = 0;
    HIPCHK(hipSetDevice(p->device));
    int rc;
    if ((rc = pool_compact(p))) return rc;
    if ((rc = p->gzWin.reserve(kasa_gunzip::HIST)) || (rc = p->gzTmp.reserve(kasa_gunzip::HIST)) || (rc = p->status.reserve(64))) return rc;
    kasa_parser::GzState s = p->gz;
    auto bad = [&](int code) { p->inflateCode = code; p->inflateMember = s.member; return refuse(p, KASA_PARSE_INFLATE, s.member, parsable); };
    static const uint32_t chunkBytes = [] { const char *e = getenv("KASA_GUNZIP_CHUNK"); const long v = e ? atol(e) : 0; return v >= (long)kasa_gunzip::MIN_CHUNK ? (uint32_t)v : kasa_gunzip::DEFAULT_CHUNK; }();
    GunzipIntoParser be;
    be.stream = p->stream; be.p = p; be.base = p->carry;
    HIPCHK(hipEventRecord(p->ev[0], p->stream));
    HIPCHK(hipEventRecord(p->evz[0], p->stream));
    if (nBytes) {
        if ((rc = p->zStream.reserve(nBytes + 8))) return rc;
        HIPCHK(hipMemcpyAsync(p->zStream.p, span, nBytes, hipMemcpyHostToDevice, p->stream));
        HIPCHK(hipEventRecord(p->evz[0], p->stream));
    }
    be.dStream = p->zStream.as<uint8_t>(); be.nBytes = (uint32_t)nBytes;
    kasa_gunzip::Stats st;
    std::memset(&st, 0, sizeof st);
    uint64_t at = 0, textN = 0;
    uint64_t lastStart = 0; bool lastFresh = s.phase != 1;    // the member that is open at the end: where its text of this span begins, and whether it began in this span
    for (;;) {
        if (s.phase == 0) {
            if (at == nBytes) break;
            uint64_t dataAt = 0;
            const int hs = kasa_gunzip::member_header(span, nBytes, at, &dataAt);
            if (hs == KASA_INFLATE_CUT && !final) break;
            if (hs != KASA_INFLATE_OK) return bad(hs);
            at = dataAt;
            s.phase = 1; s.bit = 0; s.crcReg = 0xFFFFFFFFu; s.winLen = 0; s.memberBytes = 0;
            lastStart = textN; lastFresh = true;
        }
        if (s.phase == 1) {
            int zs = KASA_INFLATE_OK; uint64_t endBit = 0, n = 0; bool ended = false;
            be.dPrev = p->gzWin.as<uint8_t>(); be.prevLen = s.winLen;
            if ((rc = kasa_gunzip::inflate_stream(be, nBytes, 8 * at + s.bit, chunkBytes, s.winLen, textN, ~0ull, !final, st, &zs, &endBit, &n, &ended))) return rc;
            if (zs != KASA_INFLATE_OK) return bad(zs);
            if (n) {
                be.dText = p->text.as<uint8_t>() + p->carry;
                if ((rc = be.crc_reg(textN, n, s.crcReg, &s.crcReg))) return rc;
            }
            textN += n; s.memberBytes += n;
            if (!ended) { at = endBit >> 3; s.bit = (uint32_t)(endBit & 7u); break; }
            at = (endBit + 7) >> 3; s.bit = 0; s.phase = 2;
        }
        if (s.phase == 2) {
            if (nBytes - at < 8) { if (final) return bad(KASA_INFLATE_CUT); break; }
            const uint8_t *t = span + at;
            const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
            const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
            if (~s.crcReg != crc) return bad(KASA_INFLATE_CRC);
            if ((uint32_t)s.memberBytes != isize) return bad((uint32_t)s.memberBytes < isize ? KASA_INFLATE_SHORT : KASA_INFLATE_OVERRUN);
            at += 8; s.phase = 0; ++s.member; ++st.members; s.winLen = 0;
        }
    }
    if (final && s.phase != 0) return bad(s.phase == 1 ? KASA_INFLATE_TRUNCATED : KASA_INFLATE_CUT);
    // no whole block in a span of the limit's size: the host path takes the file
    if (at == 0 && textN == 0 && !final && nBytes >= KASA_GZIP_SPAN_LIMIT) return bad(KASA_INFLATE_SPAN);
    const uint64_t total = p->carry + textN;
    if (total >= MAX_CHUNK) return refuse(p, KASA_PARSE_TOO_LARGE, 0, parsable);
    uint64_t added = 0, cutBytes = 0, rest = 0;
    uint8_t *text = p->text.as<uint8_t>();
    if (total) {
        const size_t padded = (size_t)((total + TILE_BYTES - 1) / TILE_BYTES) * TILE_BYTES + 64;
        if ((rc = grow_keep(p->text, padded, (size_t)total, p->stream))) return rc;
        text = p->text.as<uint8_t>();
        HIPCHK(hipMemsetAsync(text + total, 0, padded - total, p->stream));
    }
    HIPCHK(hipEventRecord(p->evz[1], p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, p->ev[0], p->evz[0]) == hipSuccess) p->msUpload += ms;
    if (hipEventElapsedTime(&ms, p->evz[0], p->evz[1]) == hipSuccess) p->msInflate += ms;
    if (total && (textN || final)) {                                             // (nothing new: the carry waits as it is)
        TextCut cut;
        cut.final = final != 0;
        int ok = 1;
        if ((rc = append_device(p, total, 0, 0, fasta, &cut, &added, &ok))) return rc;
        if (!ok) { if (parsable) *parsable = 0; return KASA_OK; }                  // (carry and stream state are where they were)
        cutBytes = cut.cutBytes; rest = total - cutBytes;
    }
    // ---- the window of the member that is still open: the last 32 KiB of its text, for the next span's first chunk
    if (s.phase == 1) {
        const uint64_t n = textN - lastStart;                                       // its text in this span
        const uint8_t *src = text + p->carry + lastStart;
        uint8_t *win = p->gzWin.as<uint8_t>();
        const uint32_t H = kasa_gunzip::HIST;
        if (n >= H) { HIPCHK(hipMemcpyAsync(win, src + (n - H), H, hipMemcpyDeviceToDevice, p->stream)); s.winLen = H; }
        else if (n) {
            const uint32_t keep = lastFresh ? 0u : (uint32_t)std::min<uint64_t>(p->gz.winLen, H - n);
            if (keep) {                                                             // (the old window moves down by n: by way of a buffer)
                HIPCHK(hipMemcpyAsync(p->gzTmp.p, win + (H - keep), keep, hipMemcpyDeviceToDevice, p->stream));
                HIPCHK(hipMemcpyAsync(win + (H - n - keep), p->gzTmp.p, keep, hipMemcpyDeviceToDevice, p->stream));
            }
            HIPCHK(hipMemcpyAsync(win + (H - n), src, n, hipMemcpyDeviceToDevice, p->stream));
            s.winLen = keep + (uint32_t)n;
        } else if (lastFresh) s.winLen = 0;
        HIPCHK(hipStreamSynchronize(p->stream));
    }
    // ---- what lies behind the cut moves to the front
    if (rest && cutBytes) {
        if (rest <= cutBytes) HIPCHK(hipMemcpyAsync(text, text + cutBytes, rest, hipMemcpyDeviceToDevice, p->stream));
        else {
            if ((rc = p->carryTmp.reserve(rest))) return rc;
            HIPCHK(hipMemcpyAsync(p->carryTmp.p, text + cutBytes, rest, hipMemcpyDeviceToDevice, p->stream));
            HIPCHK(hipMemcpyAsync(text, p->carryTmp.p, rest, hipMemcpyDeviceToDevice, p->stream));
        }
        HIPCHK(hipStreamSynchronize(p->stream));
    }
    p->carry = rest;
    p->gz = s;
    const uint64_t v[8] = {st.chunks, st.withStart, st.confirmed, st.rejected, st.rounds, st.markers, st.reruns, st.members};
    for (int i = 0; i < 8; ++i) { if (i == 4) p->gzStats[i] = std::max(p->gzStats[i], v[i]); else p->gzStats[i] += v[i]; }
    if (nReadsAdded) *nReadsAdded = added;
    if (nTextBytes) *nTextBytes = cutBytes;
    if (keepFrom) *keepFrom = at;
    return KASA_OK;
}

static int pool_ends(kasa_parser *p, uint64_t r0, uint64_t n, uint64_t (&e)[4])
{
    const PoolArrays &a = p->arrays[p->cur];
    int rc = p->status.reserve(64);
    if (rc) return rc;
    uint64_t *d = p->status.as<uint64_t>() + 2;                                   // (behind the status word)
    prs_ends_kernel<<<1, 1, 0, p->stream>>>(a.off.as<int64_t>(), a.nameOff.as<uint64_t>(), r0, n, d);
    HIPCHK(hipGetLastError());
    return fetch(p->stream, e, d);
}

static int fetch_impl(kasa_parser *p, uint64_t first, uint64_t n, uint32_t *lengths, uint64_t *nameOff, char *names, int64_t *off, uint8_t *bases)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    const uint64_t pooled = p->nReads - p->head;
    if (first > pooled || n > pooled - first)
        return fail(KASA_E_ARG, "kasa_parse_fetch: reads [%llu, +%llu) outside the %llu pooled", (unsigned long long)first, (unsigned long long)n, (unsigned long long)pooled);
    HIPCHK(hipSetDevice(p->device));
    const PoolArrays &a = p->arrays[p->cur];
    const uint64_t r0 = p->head + first;
    // the ends of the range, needed for the sizes of names and bases: one 32-byte read-back
    uint64_t e[4] = {0, 0, 0, 0};
    int rc = pool_ends(p, r0, n, e);
    if (rc) return rc;
    const int64_t ob[2] = {(int64_t)e[0], (int64_t)e[1]}; const uint64_t nb[2] = {e[2], e[3]};
    if (lengths && n) HIPCHK(hipMemcpy(lengths, a.lengths.as<uint32_t>() + r0, n * 4, hipMemcpyDeviceToHost));
    if (nameOff) { HIPCHK(hipMemcpy(nameOff, a.nameOff.as<uint64_t>() + r0, (n + 1) * 8, hipMemcpyDeviceToHost)); for (uint64_t i = 0; i <= n; ++i) nameOff[i] -= nb[0]; }
    if (off) { HIPCHK(hipMemcpy(off, a.off.as<int64_t>() + r0, (n + 1) * 8, hipMemcpyDeviceToHost)); for (uint64_t i = 0; i <= n; ++i) off[i] -= ob[0]; }
    if (names && nb[1] > nb[0]) HIPCHK(hipMemcpy(names, a.names.as<char>() + nb[0], nb[1] - nb[0], hipMemcpyDeviceToHost));
    if (bases && ob[1] > ob[0]) HIPCHK(hipMemcpy(bases, a.bases.as<uint8_t>() + ob[0], (size_t)(ob[1] - ob[0]), hipMemcpyDeviceToHost));
    return KASA_OK;
}

static int take_impl(kasa_parser *p, kasa_ctx *c, uint64_t n)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (!c) return fail(KASA_E_ARG, "ctx is NULL");
    if (c->ix->device != p->device) return fail(KASA_E_ARG, "kasa_parse_take: the context is on device %d, the pool on device %d", c->ix->device, p->device);
    if (n > p->nReads - p->head) return fail(KASA_E_ARG, "kasa_parse_take: %llu reads asked for, %llu pooled", (unsigned long long)n, (unsigned long long)(p->nReads - p->head));
    HIPCHK(hipSetDevice(p->device));
    const PoolArrays &a = p->arrays[p->cur];
    uint64_t e[4] = {0, 0, 0, 0};                                                  // where the reads left behind start: one 32-byte read-back
    int rc0 = pool_ends(p, p->head, n, e);
    if (rc0) return rc0;
    const uint64_t end = e[1], nameEnd = e[3];
    // the context copies the bases (the pool's memory is reused by the next append) and returns with its stream idle
    const int rc = upload_impl(c, a.bases.as<uint8_t>(), a.off.as<int64_t>() + p->head, (int64_t)n, nullptr, (int64_t)n, true, true);
    if (rc) return rc;
    uint64_t recEnd = p->headRec;
    if (p->keepRecords) {
        // ... and the records with their offsets, rebased, on the context's stream (the pool's is idle)
        if ((rc0 = fetch(p->stream, recEnd, a.recOff.as<uint64_t>() + p->head + n))) return rc0;
        const uint64_t nr = recEnd - p->headRec;
        if ((rc0 = c->fltRecords.reserve(nr + 64)) || (rc0 = c->fltRecOff.reserve((n + 1) * 8))) return rc0;
        if (nr) HIPCHK(hipMemcpyAsync(c->fltRecords.p, a.records.as<char>() + p->headRec, nr, hipMemcpyDeviceToDevice, c->stream));
        prs_rebase_kernel<uint64_t><<<blocks_for(n + 1, 256), 256, 0, c->stream>>>(a.recOff.as<uint64_t>() + p->head, c->fltRecOff.as<uint64_t>(), n + 1, p->headRec);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
        c->fltHaveRecords = true; c->fltRecBytes = nr;
    }
    p->head += n; p->headBase = end; p->headName = nameEnd; p->headRec = recEnd;
    return KASA_OK;
}

static int keep_records_impl(kasa_parser *p, int keep)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (p->nReads != p->head || p->carry)
        return fail(KASA_E_STATE, "kasa_pool_keep_records: %llu reads are pooled and %llu bytes carried; the pool must be empty", (unsigned long long)(p->nReads - p->head), (unsigned long long)p->carry);
    HIPCHK(hipSetDevice(p->device));
    if (keep)
        for (PoolArrays &a : p->arrays) {                                          // recOff[0] = 0
            int rc = a.recOff.reserve(8);
            if (rc) return rc;
            HIPCHK(hipMemsetAsync(a.recOff.p, 0, 8, p->stream));
        }
    HIPCHK(hipStreamSynchronize(p->stream));
    p->keepRecords = keep != 0; p->headRec = p->endRec = 0;
    return KASA_OK;
}

static int fetch_records_impl(kasa_parser *p, uint64_t first, uint64_t n, uint64_t *recOff, char *records)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (!p->keepRecords) return fail(KASA_E_STATE, "kasa_pool_fetch_records: the pool keeps no records (kasa_pool_keep_records)");
    const uint64_t pooled = p->nReads - p->head;
    if (first > pooled || n > pooled - first)
        return fail(KASA_E_ARG, "kasa_pool_fetch_records: reads [%llu, +%llu) outside the %llu pooled", (unsigned long long)first, (unsigned long long)n, (unsigned long long)pooled);
    HIPCHK(hipSetDevice(p->device));
    const PoolArrays &a = p->arrays[p->cur];
    const uint64_t r0 = p->head + first;
    uint64_t e[2] = {0, 0};
    int rc;
    if ((rc = fetch_async(p->stream, e[0], a.recOff.as<uint64_t>() + r0)) || (rc = fetch(p->stream, e[1], a.recOff.as<uint64_t>() + r0 + n))) return rc;
    if (recOff) { HIPCHK(hipMemcpy(recOff, a.recOff.as<uint64_t>() + r0, (n + 1) * 8, hipMemcpyDeviceToHost)); for (uint64_t i = 0; i <= n; ++i) recOff[i] -= e[0]; }
    if (records && e[1] > e[0]) HIPCHK(hipMemcpy(records, a.records.as<char>() + e[0], e[1] - e[0], hipMemcpyDeviceToHost));
    return KASA_OK;
}

// ---- pairs ----
static int pair_check(const char *who, kasa_parser *p, kasa_parser *q)
{
    if (!p || !q) return fail(KASA_E_ARG, "%s: a parser is NULL", who);
    if (p == q) return fail(KASA_E_ARG, "%s: both mates from one pool", who);
    if (p->device != q->device) return fail(KASA_E_ARG, "%s: the pools are on devices %d and %d", who, p->device, q->device);
    return KASA_OK;
}

// the closed-form offsets of pairs [r1, r1 + n) / [r2, r2 + n) of the two pools, letters and names (e1, e2: pool_ends of those ranges)
static void pair_offsets(const kasa_parser *p, const kasa_parser *q, uint64_t r1, uint64_t r2, const uint64_t (&e1)[4], const uint64_t (&e2)[4],
                         PairOffsets &letters, PairOffsets &names)
{
    const PoolArrays &a = p->arrays[p->cur], &b = q->arrays[q->cur];
    letters = PairOffsets{reinterpret_cast<const uint64_t *>(a.off.as<int64_t>()) + r1, reinterpret_cast<const uint64_t *>(b.off.as<int64_t>()) + r2, e1[0], e2[0]};
    names = PairOffsets{a.nameOff.as<uint64_t>() + r1, b.nameOff.as<uint64_t>() + r2, e1[2], e2[2]};
}

template <class Offsets>
static int gather64(const uint8_t *src1, const uint8_t *src2, const Offsets &d, uint64_t nEntries, uint64_t total, uint8_t *out, hipStream_t stream)
{
    if (nEntries == 0 || total == 0) return KASA_OK;
    const uint64_t tiles = (total + TILE_BYTES - 1) / TILE_BYTES;
    if (tiles / WAVES >= 0x7FFFFFFFull) return fail(KASA_E_LIMIT, "kasa_pair: %llu bytes in one call", (unsigned long long)total);
    pair_gather_kernel<Offsets><<<blocks_for(tiles, WAVES), 64 * WAVES, 0, stream>>>(src1, src2, d, nEntries, total, out);
    HIPCHK(hipGetLastError());
    return KASA_OK;
}
static int pair_gather(const uint8_t *src1, const uint8_t *src2, const PairOffsets &d, uint64_t n, uint64_t total, uint8_t *out, hipStream_t stream)
{
    return gather64(src1, src2, d, 2 * n, total, out, stream);
}

static int pair_fetch_impl(kasa_parser *p, kasa_parser *q, uint64_t first, uint64_t n, uint32_t *lengths, uint64_t *nameOff, char *names, int64_t *off, uint8_t *bases)
{
    int rc = pair_check("kasa_pair_fetch", p, q);
    if (rc) return rc;
    const uint64_t pooled = std::min(p->nReads - p->head, q->nReads - q->head);
    if (first > pooled || n > pooled - first)
        return fail(KASA_E_ARG, "kasa_pair_fetch: pairs [%llu, +%llu) outside the %llu pooled", (unsigned long long)first, (unsigned long long)n, (unsigned long long)pooled);
    HIPCHK(hipSetDevice(p->device));
    uint64_t e1[4] = {0, 0, 0, 0}, e2[4] = {0, 0, 0, 0};
    if ((rc = pool_ends(p, p->head + first, n, e1)) || (rc = pool_ends(q, q->head + first, n, e2))) return rc;
    const uint64_t nBases = (e1[1] - e1[0]) + (e2[1] - e2[0]), nNames = (e1[3] - e1[2]) + (e2[3] - e2[2]);
    const PoolArrays &a = p->arrays[p->cur], &b = q->arrays[q->cur];
    PairOffsets dl, dn;
    pair_offsets(p, q, p->head + first, q->head + first, e1, e2, dl, dn);
    if ((off && (rc = p->pairOff.reserve((2 * n + 1) * 8))) || (nameOff && (rc = p->pairNameOff.reserve((n + 1) * 8))) || (lengths && (rc = p->pairLengths.reserve(n * 4 + 64))) ||
        (names && (rc = p->pairNames.reserve(nNames + 64))) || (bases && (rc = p->pairBases.reserve(nBases + 64))))
        return rc;
    // the second pool's stream is idle (every call on a pool returns so): all of it runs on the first one's
    if (off || nameOff || lengths) {
        pair_layout_kernel<<<blocks_for(n + 1, 256), 256, 0, p->stream>>>(dl, dn, a.lengths.as<uint32_t>() + p->head + first, b.lengths.as<uint32_t>() + q->head + first, n,
            off ? p->pairOff.as<int64_t>() : nullptr, nullptr, nameOff ? p->pairNameOff.as<uint64_t>() : nullptr, lengths ? p->pairLengths.as<uint32_t>() : nullptr);
        HIPCHK(hipGetLastError());
    }
    if ((names && (rc = pair_gather(a.names.as<uint8_t>(), b.names.as<uint8_t>(), dn, n, nNames, p->pairNames.as<uint8_t>(), p->stream))) ||
        (bases && (rc = pair_gather(a.bases.as<uint8_t>(), b.bases.as<uint8_t>(), dl, n, nBases, p->pairBases.as<uint8_t>(), p->stream))))
        return rc;
    if (off) HIPCHK(hipMemcpyAsync(off, p->pairOff.p, (2 * n + 1) * 8, hipMemcpyDeviceToHost, p->stream));
    if (nameOff) HIPCHK(hipMemcpyAsync(nameOff, p->pairNameOff.p, (n + 1) * 8, hipMemcpyDeviceToHost, p->stream));
    if (lengths && n) HIPCHK(hipMemcpyAsync(lengths, p->pairLengths.p, n * 4, hipMemcpyDeviceToHost, p->stream));
    if (names && n && nNames) HIPCHK(hipMemcpyAsync(names, p->pairNames.p, nNames, hipMemcpyDeviceToHost, p->stream));
    if (bases && n && nBases) HIPCHK(hipMemcpyAsync(bases, p->pairBases.p, nBases, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return KASA_OK;
}

// The first n reads of both pools become the context's batch of n reads in 2n sequences.  The context's own buffers are
// written by the two kernels (offsets and read ids; the letters, in their one pass), upload_tail does the rest and returns
// with the stream idle: the pools' memory is free for the next append.  The heads move only when all of it went well.
static int pair_take_impl(kasa_parser *p, kasa_parser *q, kasa_ctx *c, uint64_t n)
{
    int rc = pair_check("kasa_pair_take", p, q);
    if (rc) return rc;
    if (!c) return fail(KASA_E_ARG, "ctx is NULL");
    if (c->ix->device != p->device) return fail(KASA_E_ARG, "kasa_pair_take: the context is on device %d, the pools on device %d", c->ix->device, p->device);
    if (n > p->nReads - p->head || n > q->nReads - q->head)
        return fail(KASA_E_ARG, "kasa_pair_take: %llu pairs asked for, %llu and %llu reads pooled", (unsigned long long)n, (unsigned long long)(p->nReads - p->head),
                    (unsigned long long)(q->nReads - q->head));
    HIPCHK(hipSetDevice(p->device));
    uint64_t e1[4] = {0, 0, 0, 0}, e2[4] = {0, 0, 0, 0};                           // one 32-byte read-back per pool
    if ((rc = pool_ends(p, p->head, n, e1)) || (rc = pool_ends(q, q->head, n, e2))) return rc;
    const uint64_t nBases = (e1[1] - e1[0]) + (e2[1] - e2[0]);
    const int64_t nSeq = (int64_t)(2 * n);
    if ((rc = upload_reset(c, nSeq, (int64_t)n)) || (rc = c->bases.reserve(nBases + 64)) || (rc = upload_reserve(c, nSeq, (int64_t)n))) return rc;
    const PoolArrays &a = p->arrays[p->cur], &b = q->arrays[q->cur];
    PairOffsets dl, dn;
    pair_offsets(p, q, p->head, q->head, e1, e2, dl, dn);
    pair_layout_kernel<<<blocks_for(n + 1, 256), 256, 0, c->stream>>>(dl, dn, nullptr, nullptr, n, c->rawOff.as<int64_t>(), c->seqRead.as<uint32_t>(), nullptr, nullptr);
    HIPCHK(hipGetLastError());
    if ((rc = pair_gather(a.bases.as<uint8_t>(), b.bases.as<uint8_t>(), dl, n, nBases, c->bases.as<uint8_t>(), c->stream))) return rc;
    c->basesPtr = c->bases.as<uint8_t>();
    c->haveSeqRead = true;
    if ((rc = upload_tail(c, nSeq, nullptr, (int64_t)n, nBases))) return rc;
    p->head += n; p->headBase = e1[1]; p->headName = e1[3];
    q->head += n; q->headBase = e2[1]; q->headName = e2[3];
    return KASA_OK;
}

}  // namespace kasa_parse_impl

extern "C" int kasa_parse_tile_bytes(void) { return kasa_parse_impl::TILE_BYTES; }

static int parse_create_impl(int device, uint64_t longSequence, kasa_parser **out)
{
    if (!out) return fail(KASA_E_ARG, "kasa_parse_create: out is NULL");
    *out = nullptr;
    if (longSequence == 0) return fail(KASA_E_ARG, "kasa_parse_create: longSequence must be at least 1");
    int ndev = 0;
    kasa_device_count(&ndev);
    if (device < 0 || device >= ndev) return fail(KASA_E_HIP, "kasa_parse_create: no HIP device %d (found %d)", device, ndev);
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<kasa_parser, void (*)(kasa_parser *)> p(new kasa_parser, kasa_parse_destroy);
    p->device = device; p->longSeq = longSequence;
    HIPCHK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    for (hipEvent_t &e : p->ev) HIPCHK(hipEventCreate(&e));
    for (hipEvent_t &e : p->evz) HIPCHK(hipEventCreate(&e));
    for (kasa_parse_impl::PoolArrays &a : p->arrays) {                  // off[0] = nameOff[0] = 0
        int rc;
        if ((rc = a.off.reserve(8)) || (rc = a.nameOff.reserve(8))) return rc;
        HIPCHK(hipMemsetAsync(a.off.p, 0, 8, p->stream));
        HIPCHK(hipMemsetAsync(a.nameOff.p, 0, 8, p->stream));
    }
    HIPCHK(hipStreamSynchronize(p->stream));
    *out = p.release();
    return KASA_OK;
}

extern "C" int kasa_parse_create(int device, uint64_t longSequence, kasa_parser **out) { KASA_GUARDED(parse_create_impl(device, longSequence, out)) }

extern "C" void kasa_parse_destroy(kasa_parser *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    for (hipEvent_t e : p->ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->evz) if (e) (void)hipEventDestroy(e);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

extern "C" int kasa_parse_append(kasa_parser *p, const char *text, uint64_t nBytes, int fasta, uint64_t *nReadsAdded, int *parsable)
{
    KASA_GUARDED(kasa_parse_impl::append_impl(p, text, nBytes, fasta, nReadsAdded, parsable))
}

extern "C" int kasa_bgzf_parse_append(kasa_parser *p, const void *members, uint64_t nBytes, int fasta, int final, uint64_t *nReadsAdded, int *parsable,
                                      uint64_t *nTextBytes, uint64_t *carryBytes)
{
    KASA_GUARDED(kasa_parse_impl::append_bgzf_impl(p, static_cast<const uint8_t *>(members), nBytes, fasta, final, nReadsAdded, parsable, nTextBytes, carryBytes))
}

extern "C" int kasa_gzip_parse_append(kasa_parser *p, const void *bytes, uint64_t nBytes, int fasta, int final, uint64_t *nReadsAdded, int *parsable,
                                      uint64_t *nTextBytes, uint64_t *keepFrom)
{
    KASA_GUARDED(kasa_parse_impl::append_gzip_impl(p, static_cast<const uint8_t *>(bytes), nBytes, fasta, final, nReadsAdded, parsable, nTextBytes, keepFrom))
}

extern "C" int kasa_gzip_parse_status(kasa_parser *p, int *code, uint64_t *member, uint64_t *stats8)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (code) *code = p->inflateCode;
    if (member) *member = p->inflateMember;
    if (stats8) std::memcpy(stats8, p->gzStats, sizeof p->gzStats);
    return KASA_OK;
}

extern "C" int kasa_gzip_parse_ms(kasa_parser *p, double *inflateMs)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (inflateMs) *inflateMs = p->msInflate;
    return KASA_OK;
}

extern "C" int kasa_bgzf_parse_status(kasa_parser *p, int *code, uint64_t *member)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (code) *code = p->inflateCode;
    if (member) *member = p->inflateMember;
    return KASA_OK;
}

extern "C" int kasa_bgzf_parse_ms(kasa_parser *p, double *inflateMs)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (inflateMs) *inflateMs = p->msInflate;
    return KASA_OK;
}

extern "C" int kasa_parse_status(kasa_parser *p, int *code, uint64_t *at)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (code) *code = p->lastCode;
    if (at) *at = p->lastAt;
    return KASA_OK;
}

extern "C" const char *kasa_parse_status_text(int code)
{
    switch (code) {
    case KASA_PARSE_OK: return "parsable";
    case KASA_PARSE_FASTQ_LINES: return "the line count of a FASTQ chunk is not a multiple of 4";
    case KASA_PARSE_FASTQ_HEADER: return "a FASTQ record does not start with '@'";
    case KASA_PARSE_FASTQ_PLUS: return "the third line of a FASTQ record does not start with '+'";
    case KASA_PARSE_FASTQ_QUALITY: return "a quality line differs in length from its sequence line";
    case KASA_PARSE_EMPTY_LINE: return "an empty line in a FASTQ chunk";
    case KASA_PARSE_BLANK: return "a space or tab in a sequence line";
    case KASA_PARSE_LONG: return "a sequence long enough to be read in pieces";
    case KASA_PARSE_FASTA_HEADER: return "a FASTA chunk does not start with '>'";
    case KASA_PARSE_FASTQ_SEQ_PLUS: return "a FASTQ sequence line starts with '+'";
    case KASA_PARSE_TOO_LARGE: return "a chunk of 4 GiB or more";
    case KASA_PARSE_INFLATE: return "a BGZF member that does not inflate";
    default: return "unknown";
    }
}

extern "C" int kasa_parse_sizes(kasa_parser *p, uint64_t *nReads, uint64_t *nBases, uint64_t *nNameBytes)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (nReads) *nReads = p->nReads - p->head;
    if (nBases) *nBases = p->endBase - p->headBase;
    if (nNameBytes) *nNameBytes = p->endName - p->headName;
    return KASA_OK;
}

extern "C" int kasa_parse_fetch(kasa_parser *p, uint64_t first, uint64_t n, uint32_t *lengths, uint64_t *nameOff, char *names, int64_t *off, uint8_t *bases)
{
    KASA_GUARDED(kasa_parse_impl::fetch_impl(p, first, n, lengths, nameOff, names, off, bases))
}

extern "C" int kasa_parse_take(kasa_parser *p, kasa_ctx *ctx, uint64_t nReads) { KASA_GUARDED(kasa_parse_impl::take_impl(p, ctx, nReads)) }

extern "C" int kasa_pool_keep_records(kasa_parser *p, int keep) { KASA_GUARDED(kasa_parse_impl::keep_records_impl(p, keep)) }

extern "C" int kasa_pool_fetch_records(kasa_parser *p, uint64_t first, uint64_t n, uint64_t *recOff, char *records)
{
    KASA_GUARDED(kasa_parse_impl::fetch_records_impl(p, first, n, recOff, records))
}

extern "C" int kasa_pair_take(kasa_parser *first, kasa_parser *second, kasa_ctx *ctx, uint64_t nPairs) { KASA_GUARDED(kasa_parse_impl::pair_take_impl(first, second, ctx, nPairs)) }

extern "C" int kasa_pair_fetch(kasa_parser *first, kasa_parser *second, uint64_t firstPair, uint64_t nPairs, uint32_t *lengths, uint64_t *nameOff, char *names, int64_t *off,
                               uint8_t *bases)
{
    KASA_GUARDED(kasa_parse_impl::pair_fetch_impl(first, second, firstPair, nPairs, lengths, nameOff, names, off, bases))
}

extern "C" int kasa_parse_stage_ms(kasa_parser *p, double *uploadMs, double *parseMs)
{
    if (!p) return fail(KASA_E_ARG, "parser is NULL");
    if (uploadMs) *uploadMs = p->msUpload;
    if (parseMs) *parseMs = p->msParse;
    return KASA_OK;
}
