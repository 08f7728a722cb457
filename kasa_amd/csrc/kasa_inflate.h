// kasa_inflate.h -- BGZF members inflated ON THE DEVICE (the input side of kasa_bgzf.h): every member of a blocked gzip
// file is a deflate stream of its own (RFC 1951) that says how long it is (BSIZE) and how much it holds (ISIZE <= 65536).
// A host walk of the headers (walk_members) lists the members and gives member i its place in the text -- the running sum
// of ISIZE -- before a byte is decoded; inflate_kernel then works one member per wavefront and nothing is compacted.
//
// The decoder body is plain C++ (__host__ __device__, no wave intrinsics, its state in struct Dec), so the same bit reader,
// table builder, block-header parser and symbol loop run under the host's sanitizers (tools/inflate_host_check.cpp):
//   window     WINDOW bytes of the payload, reloaded (by all lanes) whenever a quarter is used up; the bit reader takes
//              bytes from it only, and zero bits behind the payload's end that a symbol consumed are INFLATE_TRUNCATED
//   header     BFINAL, BTYPE; stored: LEN / NLEN; dynamic: the code lengths through the code-length code.  Canonical
//              codes as count[] / symbol[] (the slow path, any length to 15) plus one table of the first FAST_L / FAST_D
//              bits (the fast path), zeroed and filled by all lanes, a symbol per lane
//   symbols    ONE lane decodes up to QUEUE tokens: literal | (length, distance), each with its output position, each
//              checked against the member's bounds before it is queued
//   copy       the 64 lanes store the literals, then take the matches in order, a byte per lane; the source is the member's
//              own output in global memory (L2), byte (i mod distance) of it, which is what a byte-by-byte copy gives for
//              an overlapping match.  A match whose source was written since the last barrier waits for one
//   CRC-32     every lane a slice of the output, combined as in kasa_bgzf.h (crc_mul / crc_xpow of that file)
// Bounds: loads of the payload lie in [0, payLen), stores in [0, ISIZE) of the member, a back-reference never reaches below
// its byte 0.  What is malformed gives the member a KASA_INFLATE_* code; the first such member by index is kept in one word.
//
// Included by kasa_hip.hip (behind kasa_bgzf.h) and by tools/inflate_host_check.cpp.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/kasa_hip.h"

#if defined(__HIPCC__)
#define KASA_INF_HD __host__ __device__ inline
#else
#define KASA_INF_HD inline
#endif

namespace kasa_inflate {

constexpr uint32_t MAX_ISIZE = 65536u;            // what a BGZF member holds at most
constexpr uint32_t HEADER = 18u, TRAILER = 8u;
constexpr uint32_t FAST_L = 10u, FAST_D = 8u;     // bits of the literal/length and of the distance table
constexpr uint32_t QUEUE = 128u;                  // tokens between two copies
constexpr uint32_t WINDOW = 1024u;                // payload bytes in reach of the bit reader
constexpr uint32_t RELOAD = WINDOW / 4u;          // the window moves on once this much is used up
// the longest block header: 17 bits, 19 x 3, 316 lengths of at most 7 + 7 bits; a symbol takes at most 48 bits, a refill 7 bytes
static_assert(RELOAD + (17u + 57u + 316u * 14u + 7u) / 8u + 8u <= WINDOW, "a block header fits behind the reload mark");
constexpr uint32_t N_LIT = 288u, N_DIST = 32u, N_LENS = N_LIT + N_DIST;

struct Member {
    uint64_t payload;                             // offset of the deflate data in the span
    uint64_t out;                                 // offset of the member's text: the sum of ISIZE before it
    uint32_t payLen, isize, crc, pad;
};

// Walks a span by BSIZE (the checks of bgzfMembers in the driver and formats.bgzf_members).  Whole members are listed;
// *consumed = their bytes (a span may end inside a member), *nText = their ISIZE sum.  KASA_INFLATE_HEADER where the bytes
// at *consumed are no BGZF member header or the member states more than 65536 bytes.
inline int walk_members(const uint8_t *s, uint64_t n, std::vector<Member> &tab, uint64_t *consumed, uint64_t *nText)
{
    static const uint8_t magic[4] = {0x1F, 0x8B, 8, 4}, extra[6] = {6, 0, 'B', 'C', 2, 0};
    uint64_t at = 0, text = 0;
    int rc = KASA_INFLATE_OK;
    while (at < n) {
        const uint64_t left = n - at;
        // (a cut header is judged by the bytes that are there)
        if (std::memcmp(s + at, magic, left < 4 ? (size_t)left : 4) != 0 || (left > 10 && std::memcmp(s + at + 10, extra, left - 10 < 6 ? (size_t)(left - 10) : 6) != 0)) { rc = KASA_INFLATE_HEADER; break; }
        if (left < HEADER) break;
        const uint64_t total = (uint64_t)(s[at + 16] | s[at + 17] << 8) + 1;
        if (total < HEADER + TRAILER) { rc = KASA_INFLATE_HEADER; break; }
        if (total > left) break;
        Member m;
        m.payload = at + HEADER; m.payLen = (uint32_t)(total - HEADER - TRAILER); m.out = text; m.pad = 0;
        const uint8_t *t = s + at + total - TRAILER;
        m.crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        m.isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        if (m.isize > MAX_ISIZE) { rc = KASA_INFLATE_HEADER; break; }
        tab.push_back(m);
        text += m.isize; at += total;
    }
    *consumed = at; *nText = text;
    return rc;
}

// ---- the decoder body ---------------------------------------------------------------------------------------------------
enum : uint32_t { NEED_HEADER = 0, STORED = 1, CODED = 2, DONE = 3 };

struct Dec {
    uint64_t bits;                                // the bit buffer, the next bit lowest
    uint32_t nbits, padBits;                      // bits in it; how many of them are zeros supplied behind the payload's end
    uint32_t winBase, winPos;                     // window = payload[winBase, winBase + WINDOW); the next byte to take is win[winPos]
    uint32_t inLen;                               // payload bytes
    uint32_t outPos, isize;                       // text bytes so far (queued tokens included), and what the trailer states
    uint32_t storedSrc, storedLen;                // a stored block's bytes in the payload
    uint32_t kind, final, status;
    uint32_t reload;                              // the window has to be loaded before the next byte is taken
};

struct Tables {
    uint16_t fastL[1u << FAST_L], fastD[1u << FAST_D];    // symbol << 4 | code length; 0: the code is longer (or no code)
    uint16_t countL[16], countD[16];                      // codes per length
    uint16_t symL[N_LIT], symD[N_DIST];                   // symbols in canonical order
    uint16_t code[N_LENS];                                // the canonical code of every symbol (for the fast tables)
    uint8_t lens[N_LENS];                                 // code lengths: literal/length symbols, then the distance symbols
    // cl, offs, next, all: the header parser's work space, in LDS so that the kernel has no scratch
    uint8_t cl[20];                                       // a dynamic header's code-length code
    uint16_t offs[16], next[16];                          // build_code's running places and codes per length
    uint8_t all[N_LENS];                                  // a dynamic header's lengths as they come: both sets back to back (a repeat may span them)
    uint32_t nL, nD;
};

KASA_INF_HD void dec_init(Dec &d, uint32_t inLen, uint32_t isize)
{
    d.bits = 0; d.nbits = 0; d.padBits = 0; d.winBase = 0; d.winPos = 0; d.inLen = inLen; d.outPos = 0; d.isize = isize;
    d.storedSrc = 0; d.storedLen = 0; d.kind = NEED_HEADER; d.final = 0; d.status = KASA_INFLATE_OK; d.reload = 1;
}

// the window's bytes [lane, lane + nLanes, ...): zeros behind the payload's end
KASA_INF_HD void window_load(uint8_t *win, const uint8_t *in, uint32_t inLen, uint32_t base, uint32_t lane, uint32_t nLanes)
{
    for (uint32_t i = lane; i < WINDOW; i += nLanes) win[i] = (base < inLen && i < inLen - base) ? in[base + i] : (uint8_t)0;
}

// at least 57 bits in the buffer.  A byte behind the payload (or, which the reload mark rules out, behind the window) is zeros.
KASA_INF_HD void refill(Dec &d, const uint8_t *win)
{
    while (d.nbits <= 56u) {
        uint64_t b = 0;
        if (d.winPos < WINDOW && d.winBase + d.winPos < d.inLen) b = win[d.winPos]; else d.padBits += 8u;
        ++d.winPos;
        d.bits |= b << d.nbits; d.nbits += 8u;
    }
}
KASA_INF_HD uint32_t take(Dec &d, uint32_t n)    // n <= 16 bits that a refill put there
{
    const uint32_t v = (uint32_t)d.bits & ((1u << n) - 1u);
    d.bits >>= n; d.nbits -= n;
    return v;
}
KASA_INF_HD bool ran_out(const Dec &d) { return d.nbits < d.padBits; }    // bits behind the payload's end were consumed

// the canonical code of `n` lengths: count, symbol, code.  < 0: over-subscribed, 0: complete, > 0: incomplete
// (offs, next: 16 entries of work space each -- the caller's, so that nothing here is a private array)
KASA_INF_HD int build_code(const uint8_t *lens, uint32_t n, uint16_t *count, uint16_t *symbol, uint16_t *code, uint16_t *offs, uint16_t *next)
{
    for (uint32_t l = 0; l < 16u; ++l) count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) ++count[lens[s]];
    int left = 1;
    for (uint32_t l = 1; l < 16u; ++l) { left <<= 1; left -= (int)count[l]; if (left < 0) return left; }
    offs[1] = 0; next[1] = 0;
    for (uint32_t l = 1; l < 15u; ++l) { offs[l + 1] = (uint16_t)(offs[l] + count[l]); next[l + 1] = (uint16_t)((next[l] + count[l]) << 1); }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s];
        if (l) { symbol[offs[l]++] = (uint16_t)s; code[s] = next[l]++; }
    }
    return left;
}

// a symbol of a canonical code, bit by bit: any length to 15.  -1: no such code
KASA_INF_HD int decode_slow(Dec &d, const uint16_t *count, const uint16_t *symbol)
{
    int code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16u; ++l) {
        code |= (int)((d.bits >> (l - 1u)) & 1u);
        const int c = (int)count[l];
        if (code - c < first) { d.bits >>= l; d.nbits -= l; return (int)symbol[index + (code - first)]; }
        index += c; first += c; first <<= 1; code <<= 1;
    }
    return -1;
}
KASA_INF_HD int decode_sym(Dec &d, const uint16_t *fast, uint32_t fastBits, const uint16_t *count, const uint16_t *symbol)
{
    const uint32_t e = fast[(uint32_t)d.bits & ((1u << fastBits) - 1u)];
    if (e & 15u) { d.bits >>= (e & 15u); d.nbits -= (e & 15u); return (int)(e >> 4); }
    return decode_slow(d, count, symbol);
}

KASA_INF_HD uint32_t rev16(uint32_t v, uint32_t n)
{
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
    v = ((v & 0x00FFu) << 8) | ((v >> 8) & 0x00FFu);
    return v >> (16u - n);
}
KASA_INF_HD void fast_zero(Tables &t, uint32_t lane, uint32_t nLanes)
{
    for (uint32_t i = lane; i < (1u << FAST_L); i += nLanes) t.fastL[i] = 0;
    for (uint32_t i = lane; i < (1u << FAST_D); i += nLanes) t.fastD[i] = 0;
}
// the symbols [lane, lane + nLanes, ...) of both codes enter their table (codes are prefix-free: no entry is written twice)
KASA_INF_HD void fast_fill(Tables &t, uint32_t lane, uint32_t nLanes)
{
    for (uint32_t s = lane; s < t.nL + t.nD; s += nLanes) {
        const bool dist = s >= t.nL;
        const uint32_t at = dist ? N_LIT + (s - t.nL) : s, l = t.lens[at], fb = dist ? FAST_D : FAST_L;
        if (l == 0 || l > fb) continue;
        uint16_t *tab = dist ? t.fastD : t.fastL;
        const uint16_t e = (uint16_t)((dist ? s - t.nL : s) << 4 | l);
        for (uint32_t j = rev16(t.code[at], l); j < (1u << fb); j += 1u << l) tab[j] = e;
    }
}

// both codes of a block from t.lens; puff's rules: not over-subscribed, incomplete only as a single code of one bit
KASA_INF_HD bool build_block_codes(Tables &t)
{
    int left = build_code(t.lens, t.nL, t.countL, t.symL, t.code, t.offs, t.next);
    if (left < 0 || (left > 0 && t.nL != (uint32_t)t.countL[0] + t.countL[1])) return false;
    left = build_code(t.lens + N_LIT, t.nD, t.countD, t.symD, t.code + N_LIT, t.offs, t.next);
    if (left < 0 || (left > 0 && t.nD != (uint32_t)t.countD[0] + t.countD[1])) return false;
    return true;
}

// One block header.  -> d.kind = STORED (storedSrc / storedLen are set and checked) or CODED (t.lens and the canonical codes
// are ready, the fast tables are not yet), or d.status.
KASA_INF_HD void block_header(Dec &d, Tables &t, const uint8_t *win)
{
    refill(d, win);
    d.final = take(d, 1);
    const uint32_t type = take(d, 2);
    if (ran_out(d)) { d.status = KASA_INFLATE_TRUNCATED; return; }
    if (type == 3u) { d.status = KASA_INFLATE_BTYPE; return; }
    if (type == 0u) {
        take(d, d.nbits & 7u);
        refill(d, win);
        const uint32_t len = take(d, 16), nlen = take(d, 16);
        if (ran_out(d)) { d.status = KASA_INFLATE_TRUNCATED; return; }
        if ((len ^ nlen) != 0xFFFFu) { d.status = KASA_INFLATE_STORED_LEN; return; }
        const uint32_t src = d.winBase + d.winPos - d.nbits / 8u;           // (whole bytes are left in the buffer; zeros among them lie behind inLen)
        if (src > d.inLen || len > d.inLen - src) { d.status = KASA_INFLATE_TRUNCATED; return; }
        if (len > d.isize - d.outPos) { d.status = KASA_INFLATE_OVERRUN; return; }
        d.storedSrc = src; d.storedLen = len; d.kind = STORED;
        return;
    }
    if (type == 1u) {
        for (uint32_t s = 0; s < N_LIT; ++s) t.lens[s] = (uint8_t)(s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8);
        for (uint32_t s = 0; s < N_DIST; ++s) t.lens[N_LIT + s] = 5;
        t.nL = N_LIT; t.nD = N_DIST;
        (void)build_block_codes(t);
        d.kind = CODED;
        return;
    }
    const uint32_t hlit = take(d, 5) + 257u, hdist = take(d, 5) + 1u, hclen = take(d, 4) + 4u;
    if (hlit > 286u || hdist > 30u) { d.status = ran_out(d) ? KASA_INFLATE_TRUNCATED : KASA_INFLATE_CODE_LENGTHS; return; }
    // the order of the code-length code's lengths, five bits each: 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
    const uint64_t orderLo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t orderHi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    uint8_t *cl = t.cl;
    for (uint32_t i = 0; i < 19u; ++i) cl[i] = 0;
    for (uint32_t i = 0; i < hclen; ++i) {
        refill(d, win);
        const uint32_t at = (uint32_t)((i < 12u ? orderLo >> (5u * i) : orderHi >> (5u * (i - 12u))) & 31u);
        cl[at] = (uint8_t)take(d, 3);
    }
    if (ran_out(d)) { d.status = KASA_INFLATE_TRUNCATED; return; }
    // the code-length code borrows the literal/length code's arrays; it has to be complete
    if (build_code(cl, 19, t.countL, t.symL, t.code, t.offs, t.next) != 0) { d.status = KASA_INFLATE_CODE_LENGTHS; return; }
    uint32_t i = 0;
    uint8_t *all = t.all;
    while (i < hlit + hdist) {
        refill(d, win);
        const int s = decode_slow(d, t.countL, t.symL);
        if (s < 0) { d.status = ran_out(d) ? KASA_INFLATE_TRUNCATED : KASA_INFLATE_CODE_LENGTHS; return; }
        if (s < 16) { all[i++] = (uint8_t)s; }
        else {
            uint32_t rep; uint8_t v = 0;
            if (s == 16) { if (i == 0) { d.status = KASA_INFLATE_CODE_LENGTHS; return; } v = all[i - 1]; rep = 3u + take(d, 2); }
            else if (s == 17) rep = 3u + take(d, 3);
            else rep = 11u + take(d, 7);
            if (i + rep > hlit + hdist) { d.status = ran_out(d) ? KASA_INFLATE_TRUNCATED : KASA_INFLATE_CODE_LENGTHS; return; }
            while (rep--) all[i++] = v;
        }
        if (ran_out(d)) { d.status = KASA_INFLATE_TRUNCATED; return; }
    }
    if (all[256] == 0) { d.status = KASA_INFLATE_CODE_LENGTHS; return; }    // no end-of-block code
    for (uint32_t s = 0; s < hlit; ++s) t.lens[s] = all[s];
    for (uint32_t s = 0; s < hdist; ++s) t.lens[N_LIT + s] = all[hlit + s];
    t.nL = hlit; t.nD = hdist;
    if (!build_block_codes(t)) { d.status = KASA_INFLATE_CODE_LENGTHS; return; }
    d.kind = CODED;
}

// behind a stored block's copy: the bit reader goes on at the byte after it
KASA_INF_HD void stored_done(Dec &d)
{
    d.outPos += d.storedLen;
    d.winBase = d.storedSrc + d.storedLen; d.winPos = 0; d.reload = 1;
    d.bits = 0; d.nbits = 0; d.padBits = 0;
    d.kind = d.final ? DONE : NEED_HEADER;
}

// the last block is through: the text has ISIZE bytes and the payload ends here
KASA_INF_HD void member_end(Dec &d)
{
    if (d.outPos != d.isize) { d.status = KASA_INFLATE_SHORT; return; }
    const uint32_t used = d.winBase + d.winPos - d.nbits / 8u;             // the byte behind the one that holds the last bit
    if (used != d.inLen) d.status = used > d.inLen ? KASA_INFLATE_TRUNCATED : KASA_INFLATE_TRAILING;
}

// Symbols of a coded block until QUEUE tokens are queued, the window is used up to its reload mark, the block ends or a
// status is set.  token: a literal is its byte, a match length << 16 | distance; pos[k] = where token k's first byte goes.
// A queued token has passed every check: it lies inside [0, ISIZE) and its source at or above 0.
KASA_INF_HD uint32_t decode_symbols(Dec &d, const Tables &t, const uint8_t *win, uint32_t *tok, uint16_t *pos)
{
    uint32_t n = 0;
    while (n < QUEUE && d.winPos < RELOAD) {
        refill(d, win);
        const int s = decode_sym(d, t.fastL, FAST_L, t.countL, t.symL);
        if (s < 0 || s > 285) { d.status = ran_out(d) ? KASA_INFLATE_TRUNCATED : KASA_INFLATE_SYMBOL; break; }
        if (s < 256) {
            if (ran_out(d)) { d.status = KASA_INFLATE_TRUNCATED; break; }
            if (d.outPos >= d.isize) { d.status = KASA_INFLATE_OVERRUN; break; }
            tok[n] = (uint32_t)s; pos[n] = (uint16_t)d.outPos; ++n; ++d.outPos;
            continue;
        }
        if (s == 256) {
            if (ran_out(d)) { d.status = KASA_INFLATE_TRUNCATED; break; }
            d.kind = d.final ? DONE : NEED_HEADER;
            break;
        }
        const uint32_t li = (uint32_t)s - 257u;
        uint32_t len;
        if (li < 8u) len = 3u + li;
        else if (li == 28u) len = 258u;
        else { const uint32_t eb = (li - 4u) >> 2; len = 3u + ((4u + (li & 3u)) << eb) + take(d, eb); }
        const int ds = decode_sym(d, t.fastD, FAST_D, t.countD, t.symD);
        if (ds < 0 || ds > 29) { d.status = ran_out(d) ? KASA_INFLATE_TRUNCATED : KASA_INFLATE_SYMBOL; break; }
        uint32_t dist;
        if (ds < 4) dist = 1u + (uint32_t)ds;
        else { const uint32_t eb = ((uint32_t)ds - 2u) >> 1; dist = 1u + ((2u + ((uint32_t)ds & 1u)) << eb) + take(d, eb); }
        if (ran_out(d)) { d.status = KASA_INFLATE_TRUNCATED; break; }
        if (dist > d.outPos) { d.status = KASA_INFLATE_DISTANCE; break; }
        if (len > d.isize - d.outPos) { d.status = KASA_INFLATE_OVERRUN; break; }
        tok[n] = len << 16 | dist; pos[n] = (uint16_t)d.outPos; ++n; d.outPos += len;
    }
    return n;
}

// ---- one member, serially: the decoder body with one "lane" and byte-by-byte copies (the sanitizer build; no CRC) --------
inline int inflate_member_serial(const uint8_t *in, uint32_t inLen, uint8_t *out, uint32_t isize)
{
    Dec d; Tables t;
    uint8_t win[WINDOW]; uint32_t tok[QUEUE]; uint16_t pos[QUEUE];
    std::memset(&t, 0, sizeof t);
    dec_init(d, inLen, isize);
    while (d.status == KASA_INFLATE_OK && d.kind != DONE) {
        if (d.reload || d.winPos >= RELOAD) { d.winBase += d.winPos; d.winPos = 0; d.reload = 0; window_load(win, in, inLen, d.winBase, 0, 1); }
        if (d.kind == NEED_HEADER) {
            block_header(d, t, win);
            if (d.status != KASA_INFLATE_OK) break;
            if (d.kind == STORED) { for (uint32_t i = 0; i < d.storedLen; ++i) out[d.outPos + i] = in[d.storedSrc + i]; stored_done(d); }
            else { fast_zero(t, 0, 1); fast_fill(t, 0, 1); }
            continue;
        }
        const uint32_t n = decode_symbols(d, t, win, tok, pos);
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t len = tok[k] >> 16, dist = tok[k] & 0xFFFFu, p = pos[k];
            if (!len) out[p] = (uint8_t)tok[k];
            else for (uint32_t i = 0; i < len; ++i) out[p + i] = out[p - dist + i % dist];
        }
    }
    if (d.status == KASA_INFLATE_OK) member_end(d);
    return (int)d.status;
}

#if defined(__HIPCC__)
// ---- the kernel -----------------------------------------------------------------------------------------------------------
struct Lds {
    Tables t;
    Dec d;
    uint8_t win[WINDOW];
    uint32_t tok[QUEUE];
    uint16_t pos[QUEUE];
    uint32_t crcTab[256];
    uint32_t n;
};

__device__ __forceinline__ unsigned long long status_key(uint32_t member, uint32_t code) { return ((unsigned long long)member << 8) | code; }

// One wavefront (a workgroup of 64) per member: stream[tab[m].payload ...) -> outBase[tab[m].out, + tab[m].isize).
__global__ __launch_bounds__(64) void inflate_kernel(const uint8_t *__restrict__ stream, const Member *__restrict__ tab, uint32_t nMembers,
                                                     uint8_t *outBase, unsigned long long *__restrict__ status)
{
    __shared__ Lds s;
    const uint32_t lane = threadIdx.x, m = blockIdx.x;
    if (m >= nMembers) return;
    const Member mb = tab[m];
    const uint8_t *in = stream + mb.payload;
    uint8_t *out = outBase + mb.out;
    const uint32_t inLen = mb.payLen, isize = mb.isize;
    if (lane == 0) { Dec d; dec_init(d, inLen, isize); s.d = d; }
    for (uint32_t i = lane; i < 256u; i += 64u) {
        uint32_t c = i;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kasa_bgzf::CRC_POLY : c >> 1;
        s.crcTab[i] = c;
    }
    __syncthreads();
    uint32_t fenced = 0;                                   // the member's text below this is written and visible to every lane
    for (;;) {
        const uint32_t st = s.d.status, kind = s.d.kind;
        if (st != KASA_INFLATE_OK || kind == DONE) break;
        if (s.d.reload || s.d.winPos >= RELOAD) {
            const uint32_t base = s.d.winBase + s.d.winPos;
            __syncthreads();
            window_load(s.win, in, inLen, base, lane, 64u);
            if (lane == 0) { s.d.winBase = base; s.d.winPos = 0; s.d.reload = 0; }
            __syncthreads();
        }
        if (kind == NEED_HEADER) {
            // ON THE STATE IN LDS, not on a private copy as the symbol loop below: with `Dec d = s.d; block_header(d, ...); s.d = d`
            // hipcc's gfx950 code gave valid dynamic blocks a status (test_corpus[period_level9] and [syncflush] fail then)
            if (lane == 0) block_header(s.d, s.t, s.win);
            __syncthreads();
            if (s.d.status != KASA_INFLATE_OK) break;
            if (s.d.kind == STORED) {
                const uint32_t src = s.d.storedSrc, len = s.d.storedLen, to = s.d.outPos;
                for (uint32_t i = lane; i < len; i += 64u) out[to + i] = in[src + i];
                __syncthreads();
                if (lane == 0) { Dec d = s.d; stored_done(d); s.d = d; }
            } else {
                fast_zero(s.t, lane, 64u);
                __syncthreads();
                fast_fill(s.t, lane, 64u);
            }
            __syncthreads();
            continue;
        }
        if (lane == 0) { Dec d = s.d; s.n = decode_symbols(d, s.t, s.win, s.tok, s.pos); s.d = d; }
        __syncthreads();
        const uint32_t n = s.n;
        for (uint32_t k = lane; k < n; k += 64u) { const uint32_t t = s.tok[k]; if (!(t >> 16)) out[s.pos[k]] = (uint8_t)t; }
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.tok[k]);
            const uint32_t len = t >> 16;
            if (!len) continue;
            const uint32_t dist = t & 0xFFFFu, p = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.pos[k]);
            const uint32_t src = p - dist, srcEnd = dist < len ? p : src + len;
            if (srcEnd > fenced) { __syncthreads(); fenced = p; }          // (uniform: every lane has the same token)
            for (uint32_t i = lane; i < len; i += 64u) out[p + i] = out[src + (i < dist ? i : i % dist)];
        }
        __syncthreads();
    }
    __syncthreads();
    uint32_t code = s.d.status;
    if (code == KASA_INFLATE_OK && lane == 0) { Dec d = s.d; member_end(d); s.d = d; }
    __syncthreads();
    code = s.d.status;
    if (code == KASA_INFLATE_OK) {
        // CRC-32 as in deflate_kernel: lane i takes the slice that ends (63 - i) slices before the end
        const uint32_t n = isize, sl = (n + 63u) / 64u;
        const int64_t e = (int64_t)n - (int64_t)(63u - lane) * sl, b = e - (int64_t)sl;
        uint32_t c = (b <= 0 && e > 0) ? 0xFFFFFFFFu : 0u;
        for (int64_t i = b < 0 ? 0 : b; i < e; ++i) c = s.crcTab[(c ^ out[i]) & 0xFFu] ^ (c >> 8);
        uint32_t xp = kasa_bgzf::crc_xpow(8u * sl);
        for (uint32_t dd = 1; dd < 64u; dd <<= 1) {
            const uint32_t other = (uint32_t)__shfl_down((int)c, dd, 64);
            if ((lane & (2u * dd - 1u)) == 0u) c = kasa_bgzf::crc_mul(c, xp) ^ other;
            xp = kasa_bgzf::crc_mul(xp, xp);
        }
        const uint32_t crc = n ? ~c : 0u;
        if (lane == 0 && crc != mb.crc) code = KASA_INFLATE_CRC;
    }
    if (lane == 0 && code != KASA_INFLATE_OK) atomicMin(status, status_key(m, code));
}
#endif

} // namespace kasa_inflate
