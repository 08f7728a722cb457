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
// THE DYNAMIC CODE (KASA_BGZF_DYNAMIC, BTYPE = 10): one Huffman table per stream, the same in all of its members.
//   count   count_kernel runs the same match, insert and parse (deflate_body, MODE_COUNT) over a SAMPLE of the stream's blocks and
//           adds the tokens' symbols to a histogram of 286 literal/length and 30 distance symbols (LDS, then integer atomics on
//           ONE global histogram: the order of the adds does not matter).  THE SAMPLE: with nBlk <= 64 every block; otherwise
//           the 64 blocks floor(j nBlk / 64), j = 0..63.  A block shorter than DYN_MIN is not counted (it is coded fixed).
//   build   build_kernel, one workgroup, once per stream: every symbol's count is raised to at least 1 (a block outside the
//           sample may use any of them), the symbols are ranked by (count, symbol), one lane per alphabet merges the Huffman
//           tree (two queues), limits the lengths to 15 bits the way zlib does (leaves below level 15 are lifted to it, and a leaf
//           from above moves down a level beside one of them until nothing overflows; the lengths are dealt out again by rank) -- both codes are COMPLETE,
//           their Kraft sums are exactly 1 -- and numbers the canonical codes, bit-reversed as the coder ORs them.  It also
//           writes the block header ONCE as a bit string: BFINAL = 1, BTYPE = 10, HLIT = 29, HDIST = 29, HCLEN = 15, a FIXED
//           complete code-length code (lengths 3..15 in 4 bits, 0, 1, 2 and the run-length symbols 16, 17, 18 in 5 bits; the
//           run-length symbols are never used) and the 316 lengths: at most 74 + 316 * 5 bits, 1340 and a few as a rule.
//   code    deflate_dynamic_kernel: deflate_body (MODE_DYNAMIC) with the table in LDS (316 words: code | length << 16) in place of the
//           fixed code's arithmetic.  The header bit string follows the 18 header bytes and leaves in a flush of its own before
//           the first step.  A token is up to 48 bits (15 + 5 length, 15 + 13 distance): its bits are a 64-bit value that is
//           OR-ed into up to three staging words, and the staging words hold 1024 such tokens.  The end-of-block symbol is
//           OR-ed in at the end.  The give-up rule is the fixed code's: past the stored form the member is written stored.
//           A block shorter than DYN_MIN = 2048 bytes takes the FIXED code as before (uniform per block: n decides): at the
//           fixed code's ~0.33 of per-read text its member has under 700 bytes, of which a table saves a quarter, which is what
//           the table's header costs.
// Nothing of this comes back to the host: histogram, table and header stay in device memory (struct Code).
//
// Included by kasa_hip.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

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

// ---- the dynamic code ----
constexpr int MODE_FIXED = 0, MODE_DYNAMIC = 1, MODE_COUNT = 2;     // what deflate_body does with a step's tokens (0 / 1: KASA_BGZF_FIXED / _DYNAMIC)
constexpr uint32_t N_LIT = 286u, N_DIST = 30u, N_SYM = N_LIT + N_DIST, MAX_BITS = 15u, END_OF_BLOCK = 256u;
constexpr uint32_t SAMPLE_BLOCKS = 64u;           // count_kernel's grid at most (the rule: see above)
constexpr uint32_t DYN_MIN = 2048u;               // a block of fewer bytes takes the fixed code
constexpr uint32_t HDR_BITS_MAX = 3u + 5u + 5u + 4u + 19u * 3u + N_SYM * 5u, HDR_WORDS = (HDR_BITS_MAX + 31u) / 32u;
// a token has at most 48 bits here (15 + 5 length, 15 + 13 distance); the header bit string leaves before the first step
constexpr uint32_t STAGE_WORDS_DYN = 1552u;
static_assert(STAGE_WORDS_DYN * 32u >= 127u + STEP * 48u + MAX_BITS + 7u + TRAILER * 8u + 127u, "the staging words hold a step of 48-bit tokens");
static_assert(STAGE_WORDS_DYN * 32u >= HEADER * 8u + HDR_BITS_MAX + 127u, "the staging words hold the member's and the block's header");
static_assert(STAGE_WORDS_DYN % 4u == 0u && STAGE_WORDS % 4u == 0u, "whole 16-byte units");
struct Code {                                     // one stream's, in device memory
    uint32_t hist[N_SYM];                         // count_kernel: literal/length symbols, then distance symbols
    uint32_t tab[N_SYM];                          // build_kernel: bit-reversed code | length << 16
    uint32_t hdrBits;                             //               the block header, HDR_BITS_MAX bits at most
    uint32_t hdr[HDR_WORDS];
};

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

// a match's symbols: its length code - 257 and its distance code, each with the number and the value of its extra bits
__device__ __forceinline__ void match_syms(uint32_t tok, uint32_t &lc, uint32_t &leb, uint32_t &lex, uint32_t &dc, uint32_t &deb, uint32_t &dex)
{
    const uint32_t len = tok >> 16, l = len - 3u;
    leb = 0; lex = 0;
    if (l < 8u) lc = l;
    else if (len == MAX_MATCH) lc = 28u;
    else { leb = (31u - __clz(l)) - 2u; lc = 4u * leb + 4u + ((l >> leb) & 3u); lex = l & ((1u << leb) - 1u); }
    const uint32_t d = (tok & 0xFFFFu) - 1u;
    deb = 0; dex = 0;
    if (d < 4u) dc = d;
    else { deb = (31u - __clz(d)) - 1u; dc = 2u * deb + 2u + ((d >> deb) & 1u); dex = d & ((1u << deb) - 1u); }
}

// token: a literal is its byte; a match is length << 16 | distance (distance 32768 takes bit 15).  -> bits (LSB first), count
__device__ __forceinline__ void token_bits(uint32_t tok, uint32_t &v, uint32_t &nb)
{
    if ((tok >> 16) == 0) {
        if (tok < 144u) { v = rev_bits(0x30u + tok, 8); nb = 8; } else { v = rev_bits(0x190u + (tok - 144u), 9); nb = 9; }
        return;
    }
    uint32_t lc, leb, lex, dc, deb, dex;
    match_syms(tok, lc, leb, lex, dc, deb, dex);
    if (lc < 23u) { v = rev_bits(lc + 1u, 7); nb = 7; } else { v = rev_bits(0xC0u + (lc - 23u), 8); nb = 8; }   // symbols 257..279 | 280..285
    v |= lex << nb; nb += leb;
    v |= rev_bits(dc, 5) << nb; nb += 5u;
    v |= dex << nb; nb += deb;                                    // at most 31 bits
}
// the same with a table (bit-reversed code | length << 16 of the literal/length symbols, then of the distance symbols): at most 48 bits
__device__ __forceinline__ void token_bits(uint32_t tok, const uint32_t *tab, uint64_t &v, uint32_t &nb)
{
    if ((tok >> 16) == 0) { const uint32_t e = tab[tok]; v = e & 0xFFFFu; nb = e >> 16; return; }
    uint32_t lc, leb, lex, dc, deb, dex;
    match_syms(tok, lc, leb, lex, dc, deb, dex);
    const uint32_t el = tab[257u + lc], ed = tab[N_LIT + dc];
    const uint32_t nl = (el >> 16) + leb, nd = (ed >> 16) + deb;                       // at most 20 and 28
    const uint32_t lo = (el & 0xFFFFu) | lex << (el >> 16), hi = (ed & 0xFFFFu) | dex << (ed >> 16);
    v = (uint64_t)lo | (uint64_t)hi << nl; nb = nl + nd;
}

// `nb` bits of v at bit `at` of the staging words (which start at bit `base`, a multiple of 128)
__device__ __forceinline__ void stage_or(uint32_t *stage, uint32_t base, uint32_t at, uint32_t v, uint32_t nb)
{
    const uint32_t rel = at - base, w = rel >> 5, sh = rel & 31u;
    atomicOr(&stage[w], v << sh);
    if (sh + nb > 32u) atomicOr(&stage[w + 1], v >> (32u - sh));
}
// up to 48 bits: three words at most
__device__ __forceinline__ void stage_or(uint32_t *stage, uint32_t base, uint32_t at, uint64_t v, uint32_t nb)
{
    const uint32_t rel = at - base, w = rel >> 5, sh = rel & 31u;
    const uint64_t lo = v << sh;                                   // (sh + nb <= 79: what passes bit 63 goes into the third word)
    atomicOr(&stage[w], (uint32_t)lo);
    if (sh + nb > 32u) atomicOr(&stage[w + 1], (uint32_t)(lo >> 32));
    if (sh + nb > 64u) atomicOr(&stage[w + 2], (uint32_t)(v >> (64u - sh)));          // (sh >= 17 here)
}

struct LdsMatch {                                 // what match, insert and parse need
    uint8_t in[BLOCK_IN + IN_PAD];
    uint32_t hash[HASH_N];                        // position + 1 of the most recent occurrence in earlier steps; 0: none
    uint32_t match[STEP];                         // the token a parse that stands at this position takes
    uint32_t tok[STEP];
};
template <uint32_t WORDS> struct LdsCode {        // what coding a member needs
    uint32_t stage[WORDS];
    uint32_t crcTab[256];
    uint32_t crcPart[THREADS];
    uint32_t wave[THREADS / 64u];
    uint32_t held[4];                             // bytes 16..31 of the member (BSIZE is in them)
};
static_assert(sizeof(LdsMatch) % 16u == 0u, "the staging words are read in 16-byte units");
template <int MODE> struct Lds;
template <> struct Lds<MODE_FIXED> : LdsMatch, LdsCode<STAGE_WORDS> { uint32_t nTok; };
template <> struct Lds<MODE_DYNAMIC> : LdsMatch, LdsCode<STAGE_WORDS_DYN> { uint32_t nTok; uint32_t tab[N_SYM]; };
template <> struct Lds<MODE_COUNT> : LdsMatch { uint32_t nTok; uint32_t hist[N_SYM]; };

// One block of the text (n <= BLOCK_IN bytes of it, n > 0; the text is 16-byte aligned).
//   MODE_FIXED, MODE_DYNAMIC   its member at members + block STRIDE, the member's length in sizes[block]; `code` is the stream's
//                              table and header (MODE_DYNAMIC; a block of fewer than DYN_MIN bytes is coded fixed)
//   MODE_COUNT                 its tokens' symbols and one end-of-block added to code->hist (nothing for fewer than DYN_MIN bytes)
template <int MODE>
__device__ __forceinline__ void deflate_body(Lds<MODE> &s, const uint8_t *__restrict__ text, uint64_t nTotal, uint32_t block, uint8_t *__restrict__ members,
                                             uint64_t *__restrict__ sizes, Code *__restrict__ code)
{
    constexpr bool CODED = MODE != MODE_COUNT;
    constexpr uint32_t WORDS = MODE == MODE_DYNAMIC ? STAGE_WORDS_DYN : STAGE_WORDS;
    using bits_t = std::conditional_t<MODE == MODE_DYNAMIC, uint64_t, uint32_t>;
    const uint32_t lane = threadIdx.x;
    const uint64_t first = (uint64_t)block * BLOCK_IN;
    const uint32_t n = (uint32_t)(nTotal - first < (uint64_t)BLOCK_IN ? nTotal - first : (uint64_t)BLOCK_IN);
    const uint8_t *src = text + first;
    const bool dyn = MODE == MODE_DYNAMIC && n >= DYN_MIN;        // (uniform)
    if (MODE == MODE_COUNT && n < DYN_MIN) return;
    uint8_t *member = CODED ? members + (uint64_t)block * STRIDE : nullptr;

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
    if constexpr (CODED) {
        for (uint32_t i = lane; i < WORDS; i += THREADS) s.stage[i] = 0u;
        if (lane < 256u) {
            uint32_t c = lane;
#pragma unroll
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
            s.crcTab[lane] = c;
        }
    }
    if constexpr (MODE == MODE_DYNAMIC) { if (lane < N_SYM) s.tab[lane] = code->tab[lane]; }
    if constexpr (MODE == MODE_COUNT) { if (lane < N_SYM) s.hist[lane] = 0u; }
    __syncthreads();

    // ---- CRC-32: lane i takes the slice that ends (THREADS - 1 - i) slices before the end ----
    uint32_t crc = 0;
    if constexpr (CODED) {
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

    // full 16-byte units of the staging words leave (bits [oldPos & ~127, newPos & ~127) of the member); the unit that is
    // filling moves to the front
    auto leave = [&](uint32_t oldPos, uint32_t newPos) {
        if constexpr (CODED) {
            const uint32_t u0 = oldPos >> 7, nFull = (newPos >> 7) - u0;
            if (lane < nFull) {
                const uint4 q = *reinterpret_cast<const uint4 *>(&s.stage[lane * 4u]);
                if (u0 + lane == 1u) { s.held[0] = q.x; s.held[1] = q.y; s.held[2] = q.z; s.held[3] = q.w; }
                else *reinterpret_cast<uint4 *>(member + (uint64_t)(u0 + lane) * 16u) = q;
            }
            uint32_t keep = 0;
            if (lane < 4u) keep = s.stage[nFull * 4u + lane];
            __syncthreads();
            for (uint32_t i = lane; i < WORDS; i += THREADS) s.stage[i] = i < 4u ? keep : 0u;
            __syncthreads();
        }
    };

    // ---- the member's header and the deflate block's: BFINAL = 1, BTYPE = 01 | the stream's header bit string (BTYPE = 10) ----
    uint32_t bitPos = HEADER * 8u + 3u;
    if constexpr (CODED) {
        if (lane == 0) {
            // bytes 0..15 are the same in every member: 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6, 'B' 'C' 02 00
            *reinterpret_cast<uint4 *>(member) = make_uint4(0x04088B1Fu, 0u, 0x0006FF00u, 0x00024342u);
            if (!dyn) s.stage[0] = 3u << 16;                       // bytes 16..: BSIZE (filled in last), then the 3 bits
        }
    }
    if constexpr (MODE == MODE_DYNAMIC) {
        if (dyn) {
            const uint32_t hb = code->hdrBits;                     // (<= HDR_BITS_MAX: lanes 0 .. HDR_WORDS - 1 at most)
            // (the staging words begin at byte 16 of the member, bit 128: bytes 0..15 are stored above)
            if (lane < HDR_WORDS && lane * 32u < hb) stage_or(s.stage, 128u, HEADER * 8u + lane * 32u, code->hdr[lane], hb - lane * 32u < 32u ? hb - lane * 32u : 32u);
            bitPos = HEADER * 8u + hb;
            __syncthreads();
            leave(128u, bitPos);
        }
    }
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
        const uint32_t nTok = s.nTok;
        if constexpr (MODE == MODE_COUNT) {
            // -- count: the symbols of a lane's token (the next step writes s.tok behind its first barrier) --
            if (lane < nTok) {
                const uint32_t t = s.tok[lane];
                if ((t >> 16) == 0) atomicAdd(&s.hist[t], 1u);
                else {
                    uint32_t lc, leb, lex, dc, deb, dex;
                    match_syms(t, lc, leb, lex, dc, deb, dex);
                    atomicAdd(&s.hist[257u + lc], 1u); atomicAdd(&s.hist[N_LIT + dc], 1u);
                }
            }
        } else {
            // -- code --
            bits_t v = 0; uint32_t nb = 0;
            if (lane < nTok) {
                if constexpr (MODE == MODE_DYNAMIC) {
                    if (dyn) token_bits(s.tok[lane], s.tab, v, nb);
                    else { uint32_t v32; token_bits(s.tok[lane], v32, nb); v = v32; }
                } else token_bits(s.tok[lane], v, nb);
            }
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
            leave(bitPos, newPos);
            bitPos = newPos;
        }
    }
    if constexpr (MODE == MODE_COUNT) {
        __syncthreads();
        if (lane < N_SYM) {
            const uint32_t c = s.hist[lane] + (lane == END_OF_BLOCK ? 1u : 0u);
            if (c) atomicAdd(&code->hist[lane], c);
        }
        return;
    }

    uint32_t memberBytes;
    if constexpr (CODED) {
    if (!stored) {
        uint32_t eob = 0, eobBits = 7u;                            // fixed: the end-of-block symbol is 7 zero bits, nothing to OR
        if constexpr (MODE == MODE_DYNAMIC) { if (dyn) { eob = s.tab[END_OF_BLOCK] & 0xFFFFu; eobBits = s.tab[END_OF_BLOCK] >> 16; } }
        const uint32_t dataEnd = (bitPos + eobBits + 7u) & ~7u;
        if (dataEnd > giveUp - 8u) stored = true;                  // not smaller than 5 + n bytes
        else {
            if (lane == 0) {
                const uint32_t base = bitPos & ~127u;
                if (eob) stage_or(s.stage, base, bitPos, eob, eobBits);
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
                sizes[block] = memberBytes;
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
    if (lane == 0) sizes[block] = memberBytes;
    }
}

// One member in the fixed code.  members: STRIDE bytes of scratch per block.
__global__ __launch_bounds__(1024) void deflate_kernel(const uint8_t *__restrict__ text, uint64_t nTotal, uint8_t *__restrict__ members, uint64_t *__restrict__ sizes)
{
    __shared__ __attribute__((aligned(16))) Lds<MODE_FIXED> s;
    deflate_body<MODE_FIXED>(s, text, nTotal, blockIdx.x, members, sizes, nullptr);
}
// One member in the stream's own code (build_kernel's).
__global__ __launch_bounds__(1024) void deflate_dynamic_kernel(const uint8_t *__restrict__ text, uint64_t nTotal, uint8_t *__restrict__ members, uint64_t *__restrict__ sizes, Code *__restrict__ code)
{
    __shared__ __attribute__((aligned(16))) Lds<MODE_DYNAMIC> s;
    deflate_body<MODE_DYNAMIC>(s, text, nTotal, blockIdx.x, members, sizes, code);
}
// The sampled blocks' symbols into code->hist (zeroed before).  text, nTotal: the WHOLE stream's, nBlk its blocks; the grid is
// min(nBlk, SAMPLE_BLOCKS) workgroups.
__global__ __launch_bounds__(1024) void count_kernel(const uint8_t *__restrict__ text, uint64_t nTotal, uint32_t nBlk, Code *__restrict__ code)
{
    __shared__ __attribute__((aligned(16))) Lds<MODE_COUNT> s;
    const uint32_t block = nBlk <= SAMPLE_BLOCKS ? blockIdx.x : (uint32_t)((uint64_t)blockIdx.x * nBlk / SAMPLE_BLOCKS);
    deflate_body<MODE_COUNT>(s, text, nTotal, block, nullptr, nullptr, code);
}

__device__ const uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};      // RFC 1951, 3.2.7

// ---- the table of a stream: lengths of at most MAX_BITS bits from code->hist, canonical codes, the block header ----
struct BuildLds {
    uint32_t cnt[N_SYM];                          // max(count, 1)
    uint32_t weight[N_SYM];                       // the inner nodes of an alphabet's tree in the order they are made (from the alphabet's first symbol on)
    uint16_t order[N_SYM];                        // an alphabet's symbols by (count, symbol), ascending
    uint16_t parent[2u * N_SYM];                  // of a tree's nodes: its n leaves by rank, then its n - 1 inner nodes
    uint16_t depth[2u * N_SYM];
    uint8_t len[N_SYM];
    uint32_t bl[2][MAX_BITS + 1u], next[2][MAX_BITS + 1u];        // per alphabet: symbols of a length, the next code of a length
};
// (one lane) the alphabet of n symbols from symbol `off` on: s.len, code->tab
__device__ inline void build_code(BuildLds &s, uint32_t off, uint32_t n, Code *code)
{
    uint32_t *weight = s.weight + off; uint16_t *order = s.order + off, *parent = s.parent + 2u * off, *depth = s.depth + 2u * off;
    // two queues, both ascending: the leaves by rank and the inner nodes as they are made; a leaf goes first among equals
    uint32_t li = 0, ii = 0;
    for (uint32_t k = 0; k + 1u < n; ++k) {
        uint32_t w = 0;
        for (int t = 0; t < 2; ++t) {
            if (li < n && (ii >= k || s.cnt[off + order[li]] <= weight[ii])) { w += s.cnt[off + order[li]]; parent[li++] = (uint16_t)(n + k); }
            else { w += weight[ii]; parent[n + ii++] = (uint16_t)(n + k); }
        }
        weight[k] = w;
    }
    depth[2u * n - 2u] = 0;
    for (uint32_t k = 2u * n - 2u; k-- > 0u;) depth[k] = depth[parent[k]] + 1u;       // (a parent is made after its children)
    // zlib's limit: every node below level MAX_BITS, leaf or not, counts as overflow and its leaves are lifted to that level;
    // a leaf from the deepest level above it that has one moves down a level and takes one of them as its sibling (two nodes
    // fewer overflow), until none is left over
    uint32_t *bl = s.bl[off ? 1 : 0], *next = s.next[off ? 1 : 0];
    for (uint32_t b = 0; b <= MAX_BITS; ++b) bl[b] = 0;
    int overflow = 0;
    for (uint32_t r = 0; r + 1u < 2u * n; ++r) { uint32_t d = depth[r]; if (d > MAX_BITS) { d = MAX_BITS; ++overflow; } if (r < n) ++bl[d]; }
    while (overflow > 0) {
        uint32_t b = MAX_BITS - 1u;
        while (b > 1u && bl[b] == 0u) --b;
        if (bl[b] == 0u) break;                                     // (cannot be: fewer than 2^15 leaves never fill level MAX_BITS alone)
        --bl[b]; bl[b + 1u] += 2u; --bl[MAX_BITS]; overflow -= 2;
    }
    // the rarest symbols take the longest lengths; canonical codes by (length, symbol)
    { uint32_t r = 0; for (uint32_t b = MAX_BITS; b >= 1u; --b) for (uint32_t c = 0; c < bl[b]; ++c) s.len[off + order[r++]] = (uint8_t)b; }
    { uint32_t c = 0; bl[0] = 0; for (uint32_t b = 1; b <= MAX_BITS; ++b) { c = (c + bl[b - 1u]) << 1; next[b] = c; } }
    for (uint32_t i = 0; i < n; ++i) { const uint32_t l = s.len[off + i]; code->tab[off + i] = rev_bits(next[l]++, l) | l << 16; }
}
__global__ __launch_bounds__(320) void build_kernel(Code *__restrict__ code)
{
    __shared__ BuildLds s;
    const uint32_t lane = threadIdx.x;
    const uint32_t lo = lane < N_LIT ? 0u : N_LIT, hi = lane < N_LIT ? N_LIT : N_SYM;
    if (lane < N_SYM) s.cnt[lane] = code->hist[lane] ? code->hist[lane] : 1u;
    __syncthreads();
    if (lane < N_SYM) {
        const uint32_t c = s.cnt[lane];
        uint32_t r = 0;
        for (uint32_t j = lo; j < hi; ++j) { const uint32_t cj = s.cnt[j]; r += (cj < c || (cj == c && j < lane)) ? 1u : 0u; }
        s.order[lo + r] = (uint16_t)(lane - lo);
    }
    __syncthreads();
    if (lane == 0u) build_code(s, 0u, N_LIT, code);
    if (lane == 64u) build_code(s, N_LIT, N_DIST, code);          // (another wavefront)
    __syncthreads();
    if (lane == 0u) {
        // BFINAL = 1, BTYPE = 10, HLIT = 29, HDIST = 29, HCLEN = 15; the code-length code's lengths in RFC 1951's order: 4 bits
        // for 3..15 (canonical codes 0..12), 5 bits for 0, 1, 2, 16, 17, 18 (codes 26..31); then the 316 lengths in that code
        uint64_t acc = 0; uint32_t na = 0, nw = 0, total = 0;
        auto put = [&](uint32_t v, uint32_t k) {
            acc |= (uint64_t)v << na; na += k; total += k;
            if (na >= 32u) { code->hdr[nw++] = (uint32_t)acc; acc >>= 32; na -= 32u; }
        };
        put(5u, 3u); put(N_LIT - 257u, 5u); put(N_DIST - 1u, 5u); put(15u, 4u);
        for (uint32_t i = 0; i < 19u; ++i) put(CL_ORDER[i] >= 3u && CL_ORDER[i] <= 15u ? 4u : 5u, 3u);
        for (uint32_t i = 0; i < N_SYM; ++i) { const uint32_t l = s.len[i]; if (l >= 3u) put(rev_bits(l - 3u, 4), 4u); else put(rev_bits(26u + l, 5), 5u); }
        if (na) code->hdr[nw++] = (uint32_t)acc;
        code->hdrBits = total;
    }
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
