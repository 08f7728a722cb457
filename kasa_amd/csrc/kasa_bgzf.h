// kasa_bgzf.h -- the per-read file's text compressed ON THE DEVICE into BGZF (the blocked gzip of htslib / bgzip: a plain
// multi-member .gz whose members carry their own length in a 'BC' extra subfield).  Block i of the stream covers the text's
// bytes [i 65280, (i + 1) 65280); every block is one gzip member of its own: 18 bytes of header, ONE raw deflate stream
// (RFC 1951, BFINAL = 1) in the fixed Huffman code, or stored when that is not smaller, then CRC-32 and ISIZE.
//
// One workgroup of 1024 lanes per block, the block's input staged in LDS.  The block is worked off in steps of 1024
// positions, one per lane:
//   match     the lane hashes the 4 bytes at its position and looks the hash up in a table of positions in LDS that holds
//             EARLIER steps only, verifies the candidate byte by byte (length 3..258, distance 1..32768, inside the block);
//             distance 1 is tried besides (runs: their positions are of this step and not in the table yet)
//   insert    after a barrier the step's positions go into the table with atomicMax -- the most recent position of a hash
//             wins whichever lane comes first, so the same input gives the same bytes on every run
//   parse     meanwhile lane 0 walks the step's match lengths greedily and lists the tokens
//   code      one lane per token: its bits (Huffman codes most significant bit first, extra bits least significant first),
//             a workgroup scan of the bit counts, the bits OR-ed into zeroed LDS words; full 16-byte units leave with one
//             store per lane, the unit that is still filling is carried into the next step
// The member is ONE bit stream from its first header byte on, so nothing in it needs an alignment of its own; the 16 bytes
// that hold BSIZE are held back and leave last.  CRC-32: every lane takes a slice with a byte table in LDS, the slices
// are combined in a tree by multiplying with x^(8 len) mod P (32-step shift-and-xor).
//
// Members are written at a fixed stride into a scratch buffer, their sizes are scanned (rocPRIM, in kasa_hip.hip) and
// pack_kernel puts them back to back.
//
// Included by kasa_hip.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace kasa_bgzf {

constexpr uint32_t BLOCK_IN = 65280u;             // input bytes per member (bgzip's own block size)
constexpr uint32_t STRIDE = 65536u;               // a member is never longer; members are produced at this stride
constexpr uint32_t HEADER = 18u, TRAILER = 8u;
constexpr uint32_t THREADS = 1024u, STEP = THREADS;
constexpr uint32_t HASH_BITS = 13u, HASH_N = 1u << HASH_BITS;
constexpr uint32_t MAX_MATCH = 258u, MAX_DIST = 32768u, FAR = 4096u;   // a match of 3 further away than FAR costs more than its literals
constexpr uint32_t IN_PAD = 272u;                 // zeroed bytes behind the input: a 4-byte read at any position stays inside
// bits one step can add: a token has at most 31 bits (8 + 5 length, 5 + 13 distance); 1024 tokens, the end-of-block
// symbol and the padding to a byte, the 16 bytes carried in, header + block header and trailer of a member that has one step only
constexpr uint32_t STAGE_WORDS = 1056u;
static_assert(STAGE_WORDS * 32u >= 127u + (HEADER * 8u + 3u) + STEP * 31u + 7u + 7u + TRAILER * 8u + 64u, "the staging words hold a step");
static_assert(HEADER + 5u + BLOCK_IN + TRAILER + 16u <= STRIDE, "a member, and the last unit of a coded one that is given up, stay inside the stride");
constexpr uint32_t CRC_POLY = 0xEDB88320u;

// a(x) b(x) mod P in the reflected representation (bit 31 = x^0)
__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll 4
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
__device__ __forceinline__ uint32_t crc_xpow(uint32_t e)        // x^e mod P
{
    uint32_t r = 0x80000000u, b = 0x40000000u;
    for (; e; e >>= 1) { if (e & 1u) r = crc_mul(r, b); b = crc_mul(b, b); }
    return r;
}

__device__ __forceinline__ uint32_t rev_bits(uint32_t v, uint32_t n) { return __brev(v) >> (32u - n); }

// token: a literal is its byte; a match is length << 16 | distance (distance 32768 takes bit 15).  -> bits (LSB first), count
__device__ __forceinline__ void token_bits(uint32_t tok, uint32_t &v, uint32_t &nb)
{
    const uint32_t len = tok >> 16;
    if (len == 0) {
        if (tok < 144u) { v = rev_bits(0x30u + tok, 8); nb = 8; } else { v = rev_bits(0x190u + (tok - 144u), 9); nb = 9; }
        return;
    }
    const uint32_t l = len - 3u;
    uint32_t lc, leb = 0, lex = 0;                                // length code - 257, extra bits
    if (l < 8u) lc = l;
    else if (len == MAX_MATCH) lc = 28u;
    else { leb = (31u - __clz(l)) - 2u; lc = 4u * leb + 4u + ((l >> leb) & 3u); lex = l & ((1u << leb) - 1u); }
    if (lc < 23u) { v = rev_bits(lc + 1u, 7); nb = 7; } else { v = rev_bits(0xC0u + (lc - 23u), 8); nb = 8; }   // symbols 257..279 | 280..285
    v |= lex << nb; nb += leb;
    const uint32_t d = (tok & 0xFFFFu) - 1u;
    uint32_t dc, deb = 0, dex = 0;
    if (d < 4u) dc = d;
    else { deb = (31u - __clz(d)) - 1u; dc = 2u * deb + 2u + ((d >> deb) & 1u); dex = d & ((1u << deb) - 1u); }
    v |= rev_bits(dc, 5) << nb; nb += 5u;
    v |= dex << nb; nb += deb;                                    // at most 31 bits
}

// `nb` bits of v at bit `at` of the staging words (which start at bit `base`, a multiple of 128)
__device__ __forceinline__ void stage_or(uint32_t *stage, uint32_t base, uint32_t at, uint32_t v, uint32_t nb)
{
    const uint32_t rel = at - base, w = rel >> 5, sh = rel & 31u;
    atomicOr(&stage[w], v << sh);
    if (sh + nb > 32u) atomicOr(&stage[w + 1], v >> (32u - sh));
}

struct Lds {
    uint8_t in[BLOCK_IN + IN_PAD];
    uint32_t hash[HASH_N];                        // position + 1 of the most recent occurrence in earlier steps; 0: none
    uint32_t match[STEP];                         // the token a parse that stands at this position takes
    uint32_t tok[STEP];
    uint32_t stage[STAGE_WORDS];
    uint32_t crcTab[256];
    uint32_t crcPart[THREADS];
    uint32_t wave[THREADS / 64u];
    uint32_t held[4];                             // bytes 16..31 of the member (BSIZE is in them)
    uint32_t nTok;
};

// One member.  text: the block's input (16-byte aligned, n <= BLOCK_IN bytes, n > 0); member: STRIDE bytes of scratch.
__global__ __launch_bounds__(1024) void deflate_kernel(const uint8_t *__restrict__ text, uint64_t nTotal, uint8_t *__restrict__ members, uint64_t *__restrict__ sizes)
{
    __shared__ __attribute__((aligned(16))) Lds s;
    const uint32_t lane = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * BLOCK_IN;
    const uint32_t n = (uint32_t)(nTotal - first < (uint64_t)BLOCK_IN ? nTotal - first : (uint64_t)BLOCK_IN);
    const uint8_t *src = text + first;
    uint8_t *member = members + (uint64_t)blockIdx.x * STRIDE;

    // ---- stage the input, clear the tables ----
    for (uint32_t c = lane * 16u; c < BLOCK_IN + IN_PAD; c += THREADS * 16u) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (c + 16u <= n) v = *reinterpret_cast<const uint4 *>(src + c);
        else if (c < n) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t i = 0; i < 16u; ++i) if (c + i < n) w[i >> 2] |= (uint32_t)src[c + i] << (8u * (i & 3u));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4 *>(s.in + c) = v;
    }
    for (uint32_t i = lane; i < HASH_N; i += THREADS) s.hash[i] = 0u;
    for (uint32_t i = lane; i < STAGE_WORDS; i += THREADS) s.stage[i] = 0u;
    if (lane < 256u) {
        uint32_t c = lane;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
        s.crcTab[lane] = c;
    }
    __syncthreads();

    // ---- CRC-32: lane i takes the slice that ends (THREADS - 1 - i) slices before the end ----
    uint32_t crc;
    {
        const uint32_t sl = (n + THREADS - 1u) / THREADS;
        const int64_t e = (int64_t)n - (int64_t)(THREADS - 1u - lane) * sl, b = e - (int64_t)sl;
        uint32_t c = (b <= 0 && e > 0) ? 0xFFFFFFFFu : 0u;        // the initial complement, once: where byte 0 is
        for (int64_t i = b < 0 ? 0 : b; i < e; ++i) c = s.crcTab[(c ^ s.in[i]) & 0xFFu] ^ (c >> 8);
        s.crcPart[lane] = c;
        uint32_t xp = crc_xpow(8u * sl);                          // x^(8 sl); squared from level to level
        __syncthreads();
        for (uint32_t d = 1; d < THREADS; d <<= 1) {
            uint32_t r = 0; const bool mine = (lane & (2u * d - 1u)) == 0u;
            if (mine) r = crc_mul(s.crcPart[lane], xp) ^ s.crcPart[lane + d];
            __syncthreads();
            if (mine) s.crcPart[lane] = r;
            xp = crc_mul(xp, xp);
            __syncthreads();
        }
        crc = ~s.crcPart[0];
    }

    // ---- the member's header and the deflate block's: BFINAL = 1, BTYPE = 01 ----
    if (lane == 0) {
        // bytes 0..15 are the same in every member: 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 02 00
        *reinterpret_cast<uint4 *>(member) = make_uint4(0x04088B1Fu, 0u, 0x0006FF00u, 0x00024342u);
        s.stage[0] = 3u << 16;                                     // bytes 16..: BSIZE (filled in last), then the 3 bits
    }
    uint32_t bitPos = HEADER * 8u + 3u;
    const uint32_t giveUp = (HEADER + 5u + n) * 8u;                // coded is kept only while it is smaller than stored
    bool stored = false;
    uint32_t cur = 0;                                              // (lane 0) the parse stands here
    __syncthreads();

    const uint32_t nSteps = (n + STEP - 1u) / STEP;
    for (uint32_t st = 0; st < nSteps; ++st) {
        const uint32_t p0 = st * STEP, p = p0 + lane;
        // -- match --
        uint32_t h = 0; bool hashed = false;
        if (p < n) {
            uint32_t best = 0, bestDist = 0;
            const uint32_t room = n - p < MAX_MATCH ? n - p : MAX_MATCH;
            if (p + 4u <= n) {
                const uint32_t w = (uint32_t)s.in[p] | (uint32_t)s.in[p + 1] << 8 | (uint32_t)s.in[p + 2] << 16 | (uint32_t)s.in[p + 3] << 24;
                h = (w * 2654435761u) >> (32u - HASH_BITS); hashed = true;
                const uint32_t c1 = s.hash[h];
                if (c1 != 0u && p - (c1 - 1u) <= MAX_DIST) {
                    const uint32_t c = c1 - 1u;
                    uint32_t l = 0;
                    while (l < room && s.in[c + l] == s.in[p + l]) ++l;
                    if (l >= 4u || (l == 3u && p - c <= FAR)) { best = l; bestDist = p - c; }
                }
            }
            if (p >= 1u && room >= 3u && s.in[p - 1u] == s.in[p] && bestDist != 1u) {
                uint32_t l = 1;
                while (l < room && s.in[p - 1u + l] == s.in[p + l]) ++l;
                if (l >= 3u && l >= best) { best = l; bestDist = 1u; }
            }
            s.match[lane] = best ? (best << 16 | bestDist) : (uint32_t)s.in[p];
        }
        __syncthreads();
        // -- insert (all lanes), parse (lane 0) --
        if (hashed) atomicMax(&s.hash[h], p + 1u);
        if (lane == 0) {
            const uint32_t end = p0 + STEP < n ? p0 + STEP : n;
            uint32_t k = 0;
            while (cur < end) { const uint32_t t = s.match[cur - p0]; s.tok[k++] = t; cur += (t >> 16) ? (t >> 16) : 1u; }
            s.nTok = k;
        }
        __syncthreads();
        // -- code --
        const uint32_t nTok = s.nTok;
        uint32_t v = 0, nb = 0;
        if (lane < nTok) token_bits(s.tok[lane], v, nb);
        uint32_t x = nb;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t y = __shfl_up(x, d, 64); if ((lane & 63u) >= d) x += y; }
        if ((lane & 63u) == 63u) s.wave[lane >> 6] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < THREADS / 64u; ++w) { const uint32_t t = s.wave[w]; if (w < (lane >> 6)) before += t; total += t; }
        if (bitPos + total > giveUp) { stored = true; break; }    // (uniform: every lane has the same sums)
        const uint32_t base = bitPos & ~127u;
        if (nb) stage_or(s.stage, base, bitPos + before + x - nb, v, nb);
        const uint32_t newPos = bitPos + total;
        __syncthreads();
        // -- full units leave; the unit that is filling moves to the front --
        const uint32_t u0 = bitPos >> 7, nFull = (newPos >> 7) - u0;
        if (lane < nFull) {
            const uint4 q = *reinterpret_cast<const uint4 *>(&s.stage[lane * 4u]);
            if (u0 + lane == 1u) { s.held[0] = q.x; s.held[1] = q.y; s.held[2] = q.z; s.held[3] = q.w; }
            else *reinterpret_cast<uint4 *>(member + (uint64_t)(u0 + lane) * 16u) = q;
        }
        uint32_t keep = 0;
        if (lane < 4u) keep = s.stage[nFull * 4u + lane];
        __syncthreads();
        for (uint32_t i = lane; i < STAGE_WORDS; i += THREADS) s.stage[i] = i < 4u ? keep : 0u;
        bitPos = newPos;
        __syncthreads();
    }

    uint32_t memberBytes;
    if (!stored) {
        const uint32_t dataEnd = (bitPos + 7u + 7u) & ~7u;        // the end-of-block symbol is 7 zero bits: nothing to OR
        if (dataEnd > giveUp - 8u) stored = true;                  // not smaller than 5 + n bytes
        else {
            if (lane == 0) {
                const uint32_t base = bitPos & ~127u;
                stage_or(s.stage, base, dataEnd, crc & 0xFFFFu, 16u); stage_or(s.stage, base, dataEnd + 16u, crc >> 16, 16u);
                stage_or(s.stage, base, dataEnd + 32u, n & 0xFFFFu, 16u); stage_or(s.stage, base, dataEnd + 48u, n >> 16, 16u);
            }
            const uint32_t endPos = dataEnd + TRAILER * 8u;
            memberBytes = endPos >> 3;
            __syncthreads();
            const uint32_t u0 = bitPos >> 7, nUnits = ((endPos + 127u) >> 7) - u0;
            if (lane < nUnits) {
                const uint4 q = *reinterpret_cast<const uint4 *>(&s.stage[lane * 4u]);
                if (u0 + lane == 1u) { s.held[0] = q.x; s.held[1] = q.y; s.held[2] = q.z; s.held[3] = q.w; }
                else *reinterpret_cast<uint4 *>(member + (uint64_t)(u0 + lane) * 16u) = q;
            }
            __syncthreads();
            if (lane == 0) {
                const uint4 q = make_uint4(s.held[0] | (memberBytes - 1u), s.held[1], s.held[2], s.held[3]);
                *reinterpret_cast<uint4 *>(member + 16u) = q;
                sizes[blockIdx.x] = memberBytes;
            }
            return;
        }
    }
    // ---- stored: header, 01, LEN, NLEN, the bytes, CRC-32, ISIZE -- written whole, over whatever the coded form left ----
    __syncthreads();
    memberBytes = HEADER + 5u + n + TRAILER;
    auto byteAt = [&](uint32_t j) -> uint32_t {
        const uint32_t bs = memberBytes - 1u;
        if (j >= HEADER + 5u) {
            const uint32_t i = j - (HEADER + 5u);
            if (i < n) return s.in[i];
            const uint32_t t = i - n;
            return t < 4u ? (crc >> (8u * t)) & 0xFFu : t < 8u ? (n >> (8u * (t - 4u))) & 0xFFu : 0u;
        }
        switch (j) {
        case 0: return 0x1Fu; case 1: return 0x8Bu; case 2: return 8u; case 3: return 4u;
        case 9: return 0xFFu; case 10: return 6u; case 12: return 'B'; case 13: return 'C'; case 14: return 2u;
        case 16: return bs & 0xFFu; case 17: return bs >> 8;
        case 18: return 1u;
        case 19: return n & 0xFFu; case 20: return n >> 8; case 21: return ~n & 0xFFu; case 22: return (~n >> 8) & 0xFFu;
        default: return 0u;
        }
    };
    for (uint32_t w = lane; w * 4u < memberBytes; w += THREADS)
        *reinterpret_cast<uint32_t *>(member + w * 4u) = byteAt(w * 4u) | byteAt(w * 4u + 1u) << 8 | byteAt(w * 4u + 2u) << 16 | byteAt(w * 4u + 3u) << 24;
    if (lane == 0) sizes[blockIdx.x] = memberBytes;
}

// member b: size[b] bytes at members + b STRIDE -> out + off[b].  The destination has any alignment: whole destination words
// are made of two source words.
__global__ __launch_bounds__(256) void pack_kernel(const uint8_t *__restrict__ members, const uint64_t *__restrict__ size, const uint64_t *__restrict__ off, uint8_t *__restrict__ out)
{
    const uint8_t *src = members + (uint64_t)blockIdx.x * STRIDE;
    uint8_t *dst = out + off[blockIdx.x];
    const uint32_t len = (uint32_t)size[blockIdx.x];
    uint32_t head = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u;
    if (head > len) head = len;
    const uint32_t nW = (len - head) >> 2, tail = head + nW * 4u;
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    if (threadIdx.x < len - tail) dst[tail + threadIdx.x] = src[tail + threadIdx.x];
    const uint32_t sh = (head & 3u) * 8u;                           // (src is 4-byte aligned: the stride is)
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(src) + (head >> 2);
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t w = threadIdx.x; w < nW; w += 256u) {
        const uint32_t lo = sw[w];
        dw[w] = sh ? (lo >> sh) | (sw[w + 1] << (32u - sh)) : lo;  // (sw[w + 1] reaches at most 3 bytes beyond the member: inside the stride)
    }
}

} // namespace kasa_bgzf
