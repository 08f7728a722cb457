// kasa_gunzip.h -- ONE LONG deflate stream inflated on the device: the gzip file that gzip, pigz and most download sites write
// has no BC subfield and no member table, so nothing says where a wavefront may begin.  The two-stage scheme of pugz /
// rapidgzip, a wavefront per chunk of `chunkBytes` compressed bytes:
//   find      every chunk but the first searches ITS OWN bit range for the first offset at which a dynamic block header
//             validates (block_header of kasa_inflate.h: the rules of KASA_INFLATE_CODE_LENGTHS).  64 lanes test 64 offsets on
//             the header's first 17 bits and on the code-length code's Kraft sum; only survivors build tables, one at a time
//   decode    a wavefront per chunk that has a start: whole blocks from the start to the first block boundary at or behind
//             the next candidate, into 16-bit symbols: < 256 the byte, 256 + j "byte j of the 32 KiB before my first byte".
//             Dec, Tables and the token queue are kasa_inflate.h's; the copy phase moves symbols, markers included
//   confirm   (host, one round trip per round) a candidate is true when the confirmed chunk before it ends on it; one that is
//             passed over is dropped and its predecessor decodes on in a further round.  Every round confirms or drops a chunk
//   place     symbols go to per-job buffers with a capacity; a job that needs more goes on COUNTING and is run again with what
//             it needs.  The confirmed jobs' lengths are summed on the host into text offsets
//   chain     one workgroup walks the confirmed chunks in order and writes each one's last 32 KiB of text in place: the
//             markers there point into text that the chunks before it have already made final
//   write     everything else, all chunks at once: a marker reads the final text in its predecessor's window, 16 -> 8 bits
//   CRC-32    slices of the text, each shifted to its place with crc_xpow and folded with XOR (kasa_bgzf.h's arithmetic)
// Bounds: every load of the stream is guarded by its length (the bit reader's window, peek), every symbol store by the job's
// capacity, every text store by the confirmed total; the finder never leaves its chunk; every decoder loop consumes bits.
//
// The scheduling (inflate_stream) is a template over a backend, so the host check (tools/gunzip_host_check.cpp) runs the very
// same rounds with the serial bodies below under the sanitizers, and reports the statistics the device gives.
// Included by kasa_hip.hip (behind kasa_inflate.h) and by tools/gunzip_host_check.cpp.
#pragma once
#include "kasa_inflate.h"

namespace kasa_gunzip {

using kasa_inflate::Dec;
using kasa_inflate::Tables;
using kasa_inflate::WINDOW;
using kasa_inflate::RELOAD;
using kasa_inflate::QUEUE;

constexpr uint32_t HIST = 32768u;                 // how far a back-reference reaches
constexpr uint32_t MARK = 256u;                   // symbol MARK + j: byte j of the HIST bytes before the chunk's first
constexpr uint64_t NONE = ~0ull;                  // no candidate / no stop
constexpr uint32_t DEFAULT_CHUNK = 65536u;        // compressed bytes per chunk (kasa_gzip_inflate's chunkBytes 0)
constexpr uint32_t MIN_CHUNK = 64u;
constexpr uint32_t CAP_RATIO = 8u, CAP_SLACK = 1024u;     // a job's first capacity: symbols per compressed byte, and one more small block
constexpr uint32_t MAX_JOB_SYMS = 1u << 30;       // one job's text at most
constexpr uint32_t CHAIN_THREADS = 1024u, WRITE_THREADS = 256u, WRITE_PER_THREAD = 16u, CRC_SLICE = 4096u, CRC_THREADS = 64u;

struct Job {                                      // one wavefront's work
    uint64_t startBit, stopBit;                   // from a block header at startBit to the first block boundary >= stopBit
    uint16_t *sym;
    uint32_t cap, hist;                           // symbols sym takes; how many bytes before the first one a match may reach
};
struct Result {
    uint64_t endBit;                              // the last block boundary reached
    uint32_t nSym, need;                          // symbols up to endBit; symbols up to where the decoder stopped (> cap: run again)
    uint32_t status, final;                       // what ended the decoder behind endBit (0: the stop); endBit ends the last block
    uint32_t ranOut, pad;                         // the decoder consumed bits behind the span's end: whatever `status` says, the span cut it
};
struct Seg {                                      // a confirmed chunk's symbols and their place in the member's text
    const uint16_t *sym;
    uint64_t off;
    uint32_t n, pad;
};
struct Stats { uint64_t chunks, withStart, confirmed, rejected, rounds, markers, reruns, members; };

// n <= 57 bits at bit `at` of in[0, inLen): bytes behind the end are zeros
KASA_INF_HD uint64_t peek(const uint8_t *in, uint64_t inLen, uint64_t at, uint32_t n)
{
    const uint64_t b = at >> 3;
    uint64_t v = 0;
    for (uint32_t i = 0; i < 8u; ++i) if (b + i < inLen) v |= (uint64_t)in[b + i] << (8u * i);
    return (v >> (at & 7u)) & ((1ull << n) - 1ull);
}

// the cheap tests of a dynamic block header at bit `at`: BTYPE 2, HLIT <= 29, HDIST <= 29, and a COMPLETE code-length code
KASA_INF_HD bool header_plausible(const uint8_t *in, uint64_t inLen, uint64_t at)
{
    if (at + 17u > 8u * inLen) return false;
    const uint32_t h = (uint32_t)peek(in, inLen, at, 17);
    if (((h >> 1) & 3u) != 2u || ((h >> 3) & 31u) > 29u || ((h >> 8) & 31u) > 29u) return false;
    const uint32_t hclen = ((h >> 13) & 15u) + 4u;
    if (at + 17u + 3u * hclen > 8u * inLen) return false;
    const uint64_t cl = peek(in, inLen, at + 17u, 3u * hclen);
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < hclen; ++i) { const uint32_t l = (uint32_t)(cl >> (3u * i)) & 7u; if (l) kraft += 128u >> l; }
    return kraft == 128u;
}

// the decoder at bit `at`: the window has to be loaded from byte at / 8 before start_skip takes the bits below `at`
KASA_INF_HD void dec_at(Dec &d, uint32_t inLen, uint64_t at)
{
    kasa_inflate::dec_init(d, inLen, 0xFFFFFFFFu);
    d.winBase = (uint32_t)(at >> 3);
}
KASA_INF_HD void start_skip(Dec &d, const uint8_t *win, uint64_t at) { kasa_inflate::refill(d, win); (void)kasa_inflate::take(d, (uint32_t)(at & 7u)); }
KASA_INF_HD uint64_t bit_pos(const Dec &d) { return 8ull * ((uint64_t)d.winBase + d.winPos) - d.nbits; }

// decode_symbols of kasa_inflate.h for symbols: positions of 32 bits, no ISIZE, a match may reach `hist` bytes below byte 0
KASA_INF_HD uint32_t decode_symbols16(Dec &d, const Tables &t, const uint8_t *win, uint32_t *tok, uint32_t *pos, uint32_t hist)
{
    using namespace kasa_inflate;
    uint32_t n = 0;
    while (n < QUEUE && d.winPos < RELOAD) {
        refill(d, win);
        const int s = decode_sym(d, t.fastL, FAST_L, t.countL, t.symL);
        if (s < 0 || s > 285) { d.status = ran_out(d) ? KASA_INFLATE_TRUNCATED : KASA_INFLATE_SYMBOL; break; }
        if (d.outPos >= MAX_JOB_SYMS) { d.status = KASA_INFLATE_SPAN; break; }
        if (s < 256) {
            if (ran_out(d)) { d.status = KASA_INFLATE_TRUNCATED; break; }
            tok[n] = (uint32_t)s; pos[n] = d.outPos; ++n; ++d.outPos;
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
        if (dist > d.outPos + hist) { d.status = KASA_INFLATE_DISTANCE; break; }
        tok[n] = len << 16 | dist; pos[n] = d.outPos; ++n; d.outPos += len;
    }
    return n;
}

// symbol i of a match at p: the job's own symbol, or the marker of the byte that far below its first
KASA_INF_HD uint16_t match_symbol(const uint16_t *sym, uint32_t p, uint32_t dist, uint32_t i)
{
    const int64_t src = (int64_t)p - (int64_t)dist + (int64_t)(i < dist ? i : i % dist);
    return src >= 0 ? sym[src] : (uint16_t)(MARK + HIST + src);
}

// the byte of symbol s of a chunk whose text begins at `off`: text[0, off) is final where a marker can point.  Below byte 0 lie
// the last prevLen bytes of the member's text from the spans before, at the END of prev[0, HIST).  *bad: below those
KASA_INF_HD uint8_t resolve(uint16_t s, uint64_t off, const uint8_t *text, const uint8_t *prev, uint32_t prevLen, bool *bad)
{
    if (s < MARK) return (uint8_t)s;
    const int64_t src = (int64_t)off - (int64_t)HIST + (int64_t)(s - MARK);
    if (src >= 0) return text[src];
    if (-src > (int64_t)prevLen) { *bad = true; return 0; }
    return prev[(int64_t)HIST + src];
}
// where the chain pass begins in a chunk: its last HIST bytes
KASA_INF_HD uint64_t tail_begin(uint64_t off, uint32_t n) { return n > HIST ? off + n - HIST : off; }

// ---- the serial bodies (the sanitizer build; the device backend runs the kernels below instead) ---------------------------------
inline uint64_t find_serial(const uint8_t *in, uint32_t inLen, uint64_t lo, uint64_t hi)
{
    using namespace kasa_inflate;
    Dec d; Tables t; uint8_t win[WINDOW];
    std::memset(&t, 0, sizeof t);
    for (uint64_t q = lo; q < hi; ++q) {
        if (!header_plausible(in, inLen, q)) continue;
        dec_at(d, inLen, q);
        window_load(win, in, inLen, d.winBase, 0, 1); d.reload = 0;
        start_skip(d, win, q);
        block_header(d, t, win);
        if (d.status == KASA_INFLATE_OK && d.kind == CODED) return q;
    }
    return NONE;
}

inline void decode_serial(const uint8_t *in, uint32_t inLen, const Job &job, Result &r)
{
    using namespace kasa_inflate;
    Dec d; Tables t;
    uint8_t win[WINDOW]; uint32_t tok[QUEUE], pos[QUEUE];
    std::memset(&t, 0, sizeof t);
    dec_at(d, inLen, job.startBit);
    uint32_t skip = 1;
    r.endBit = job.startBit; r.nSym = 0; r.final = 0;
    while (d.status == KASA_INFLATE_OK && d.kind != DONE) {
        if (d.reload || d.winPos >= RELOAD) {
            d.winBase += d.winPos; d.winPos = 0; d.reload = 0; window_load(win, in, inLen, d.winBase, 0, 1);
            if (skip) { start_skip(d, win, job.startBit); skip = 0; }
        }
        if (d.kind == NEED_HEADER) {
            r.endBit = bit_pos(d); r.nSym = d.outPos;
            if (r.endBit >= job.stopBit) break;
            block_header(d, t, win);
            if (d.status != KASA_INFLATE_OK) break;
            if (d.kind == STORED) {
                for (uint32_t i = 0; i < d.storedLen; ++i) if (d.outPos + i < job.cap) job.sym[d.outPos + i] = in[d.storedSrc + i];
                stored_done(d);
            } else { fast_zero(t, 0, 1); fast_fill(t, 0, 1); }
            continue;
        }
        const uint32_t n = decode_symbols16(d, t, win, tok, pos, job.hist);
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t len = tok[k] >> 16, dist = tok[k] & 0xFFFFu, p = pos[k];
            if (!len) { if (p < job.cap) job.sym[p] = (uint16_t)tok[k]; }
            else for (uint32_t i = 0; i < len && p + i < job.cap; ++i) job.sym[p + i] = match_symbol(job.sym, p, dist, i);
        }
    }
    if (d.status == KASA_INFLATE_OK && d.kind == DONE) { r.endBit = bit_pos(d); r.nSym = d.outPos; r.final = 1; }
    r.need = d.outPos; r.status = d.status; r.ranOut = ran_out(d) ? 1u : 0u; r.pad = 0;
}

// chain and write in one: the chunks in order
inline void place_serial(const Seg *segs, uint32_t nSegs, uint8_t *text, const uint8_t *prev, uint32_t prevLen, uint64_t *markers, bool *bad)
{
    for (uint32_t i = 0; i < nSegs; ++i) {
        const Seg &g = segs[i];
        for (uint32_t k = 0; k < g.n; ++k) { if (g.sym[k] >= MARK) ++*markers; text[g.off + k] = resolve(g.sym[k], g.off, text, prev, prevLen, bad); }
    }
}

// ---- the rounds ----------------------------------------------------------------------------------------------------------------
// One deflate stream that begins at bit startBit of the backend's span of nBytes; the chunks are counted from that bit's byte.
// hist0: how many bytes of the member's text precede it (the backend has them for place).  cut: the span may end inside the
// stream -- the text then ends with the last whole block (*ended = 0, *endBit = where the next one begins).  The backend:
//   void begin()                                   the symbols of the stream before are no longer needed
//   int find(dataAt, chunkBytes, nChunks, start)   start[c], c >= 1: the first candidate in chunk c's bit range, or NONE
//   int symbols(n, &p)                             room for n symbols, kept until the next stream
//   int decode(jobs, results)
//   int place(segs, textAt, total, &markers, &bad) the text of the confirmed chunks at byte textAt of the destination
// -> KASA_OK with *status: KASA_INFLATE_OK, *endBit behind the last block, *nText the stream's text, which is
// placed when the destination has `room` for it and only counted otherwise.
template <class Backend>
int inflate_stream(Backend &be, uint64_t nBytes, uint64_t startBit, uint32_t chunkBytes, uint32_t hist0, uint64_t textAt, uint64_t room, bool cut, Stats &st,
                   int *status, uint64_t *endBit, uint64_t *nText, bool *ended)
{
    const uint64_t dataAt = startBit >> 3;
    *status = KASA_INFLATE_OK; *endBit = startBit; *nText = 0; *ended = false;
    be.begin();
    const uint64_t len = nBytes - dataAt;
    const uint32_t nChunks = len ? (uint32_t)((len + chunkBytes - 1) / chunkBytes) : 1u;
    std::vector<uint64_t> start(nChunks, NONE);
    int rc;
    if (nChunks > 1 && (rc = be.find(dataAt, chunkBytes, nChunks, start))) return rc;
    start[0] = startBit;
    std::vector<uint32_t> live;                                       // chunks that have a start, in order
    for (uint32_t c = 0; c < nChunks; ++c) if (start[c] != NONE) live.push_back(c);
    st.chunks += nChunks; st.withStart += live.size();

    std::vector<Job> jobs(live.size());
    std::vector<Result> res(live.size());
    std::vector<uint8_t> dead(live.size(), 0);
    auto first_cap = [&](const Job &j) {
        const uint64_t stop = j.stopBit < 8 * nBytes ? j.stopBit : 8 * nBytes;
        const uint64_t want = ((stop - j.startBit + 7) / 8) * CAP_RATIO + CAP_SLACK;
        return (uint32_t)(want < MAX_JOB_SYMS ? want : MAX_JOB_SYMS);
    };
    // jobs `which` with their stops set: decoded, and decoded again where the capacity was too small
    auto run = [&](const std::vector<uint32_t> &which) -> int {
        std::vector<uint32_t> todo = which;
        for (int pass = 0; pass < 2 && !todo.empty(); ++pass) {
            std::vector<Job> js; std::vector<Result> rs(todo.size());
            for (uint32_t k : todo) {
                Job &j = jobs[k];
                j.cap = pass ? res[k].need : first_cap(j);
                if ((rc = be.symbols(j.cap, &j.sym))) return rc;
                js.push_back(j);
            }
            if ((rc = be.decode(js, rs))) return rc;
            std::vector<uint32_t> again;
            for (size_t i = 0; i < todo.size(); ++i) { res[todo[i]] = rs[i]; if (rs[i].need > jobs[todo[i]].cap) again.push_back(todo[i]); }
            if (!again.empty()) ++st.reruns;
            todo.swap(again);
        }
        return todo.empty() ? KASA_OK : KASA_E_STATE;                 // (the second pass has what the first one counted)
    };
    std::vector<uint32_t> all(live.size());
    for (size_t k = 0; k < live.size(); ++k) {
        all[k] = (uint32_t)k;
        jobs[k].startBit = start[live[k]]; jobs[k].stopBit = k + 1 < live.size() ? start[live[k + 1]] : NONE;
        jobs[k].sym = nullptr; jobs[k].cap = 0; jobs[k].hist = k ? HIST : hist0;
    }
    if ((rc = run(all))) return rc;

    uint64_t rounds = 1;
    std::vector<Seg> segs;
    size_t cur = 0;
    uint64_t total = 0;
    for (;;) {
        const Result &r = res[cur];
        const bool cutHere = cut && r.status != KASA_INFLATE_OK && (r.status == KASA_INFLATE_TRUNCATED || r.ranOut);
        if (r.status != KASA_INFLATE_OK && !cutHere) { *status = (int)r.status; break; }
        if (cutHere) {                                                    // the span ends inside the block behind r.endBit
            Seg g; g.sym = jobs[cur].sym; g.off = total; g.n = r.nSym; g.pad = 0;
            segs.push_back(g); total += r.nSym; ++st.confirmed;
            *endBit = r.endBit;
            break;
        }
        size_t nxt = cur + 1;
        while (nxt < live.size() && (dead[nxt] || (!r.final && jobs[nxt].startBit < r.endBit))) { if (!dead[nxt]) { dead[nxt] = 1; ++st.rejected; } ++nxt; }
        if (r.final || (nxt < live.size() && jobs[nxt].startBit == r.endBit)) {
            Seg g; g.sym = jobs[cur].sym; g.off = total; g.n = r.nSym; g.pad = 0;
            segs.push_back(g); total += r.nSym; ++st.confirmed;
            if (r.final) { *endBit = r.endBit; *ended = true; break; }
            cur = nxt;
            continue;
        }
        // the chunk stopped at a candidate that was none: on to the next one that is left
        if (++rounds > (uint64_t)nChunks + 1) return KASA_E_STATE;
        jobs[cur].stopBit = nxt < live.size() ? jobs[nxt].startBit : NONE;
        if ((rc = run(std::vector<uint32_t>(1, (uint32_t)cur)))) return rc;
    }
    if (rounds > st.rounds) st.rounds = rounds;
    if (*status != KASA_INFLATE_OK) return KASA_OK;
    *nText = total;
    if (total && total <= room) {
        bool bad = false; uint64_t markers = 0;
        if ((rc = be.place(segs, textAt, total, &markers, &bad))) return rc;
        st.markers += markers;
        if (bad) *status = KASA_INFLATE_DISTANCE;
    }
    return KASA_OK;
}

// ---- the gzip member header (RFC 1952), on the host ------------------------------------------------------------------------------
// -> KASA_INFLATE_OK and *dataAt = where the deflate data begin; KASA_INFLATE_GZIP_HEADER: the bytes are none;
// KASA_INFLATE_CUT: they end inside one
inline int member_header(const uint8_t *s, uint64_t n, uint64_t at, uint64_t *dataAt)
{
    const uint64_t left = n - at;
    static const uint8_t magic[3] = {0x1F, 0x8B, 8};
    if (std::memcmp(s + at, magic, left < 3 ? (size_t)left : 3) != 0) return KASA_INFLATE_GZIP_HEADER;
    if (left < 10) return KASA_INFLATE_CUT;
    const uint32_t flg = s[at + 3];
    if (flg & 0xE0u) return KASA_INFLATE_GZIP_HEADER;
    uint64_t p = at + 10;
    if (flg & 4u) {                                                   // FEXTRA
        if (n - p < 2) return KASA_INFLATE_CUT;
        const uint64_t xlen = (uint64_t)s[p] | (uint64_t)s[p + 1] << 8;
        p += 2;
        if (n - p < xlen) return KASA_INFLATE_CUT;
        p += xlen;
    }
    for (uint32_t f = 8u; f <= 16u; f <<= 1) {                        // FNAME, FCOMMENT: zero-terminated
        if (!(flg & f)) continue;
        while (p < n && s[p]) ++p;
        if (p >= n) return KASA_INFLATE_CUT;
        ++p;
    }
    if (flg & 2u) { if (n - p < 2) return KASA_INFLATE_CUT; p += 2; } // FHCRC
    *dataAt = p;
    return KASA_INFLATE_OK;
}

// A whole gzip file, member after member.  The backend also has
//   int crc(textAt, n, &crc)    the CRC-32 of n bytes of the destination
// cap: what the destination takes; the members behind the one that passes it are only counted (*nText is the whole text's size).
template <class Backend>
int inflate_file(Backend &be, const uint8_t *s, uint64_t nBytes, uint32_t chunkBytes, uint64_t cap, Stats &st, int *status, uint64_t *member, uint64_t *nText)
{
    uint64_t at = 0, text = 0, m = 0;
    *status = KASA_INFLATE_OK; *member = 0; *nText = 0;
    if (!nBytes) { *status = KASA_INFLATE_GZIP_HEADER; return KASA_OK; }
    while (at < nBytes) {
        *member = m;
        uint64_t dataAt = 0, endBit = 0, n = 0;
        if ((*status = member_header(s, nBytes, at, &dataAt)) != KASA_INFLATE_OK) return KASA_OK;
        const uint64_t room = text <= cap ? cap - text : 0;
        bool ended = false;
        int rc = inflate_stream(be, nBytes, 8 * dataAt, chunkBytes, 0u, text, room, false, st, status, &endBit, &n, &ended);
        if (rc) return rc;
        if (*status != KASA_INFLATE_OK) return KASA_OK;
        const bool write = n <= room;
        const uint64_t trailer = (endBit + 7) / 8;
        if (nBytes - trailer < 8) { *status = KASA_INFLATE_CUT; return KASA_OK; }
        const uint8_t *t = s + trailer;
        const uint32_t crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
        const uint32_t isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
        if (write) {
            uint32_t got = 0;
            if ((rc = be.crc(text, n, &got))) return rc;
            if (got != crc) { *status = KASA_INFLATE_CRC; return KASA_OK; }
        }
        if ((uint32_t)n != isize) { *status = (uint32_t)n < isize ? KASA_INFLATE_SHORT : KASA_INFLATE_OVERRUN; return KASA_OK; }
        text += n; at = trailer + 8; ++m; ++st.members;
    }
    *nText = text;
    return KASA_OK;
}

#if defined(__HIPCC__)
// ---- the kernels -------------------------------------------------------------------------------------------------------------------
struct FindLds { Tables t; Dec d; uint8_t win[WINDOW]; };

// One wavefront per chunk c = blockIdx.x + 1: start[c] = the first bit of [chunk begin, chunk end) at which a dynamic header validates
__global__ __launch_bounds__(64) void find_kernel(const uint8_t *__restrict__ in, uint32_t inLen, uint64_t dataAt, uint32_t chunkBytes, uint32_t nChunks,
                                                  unsigned long long *__restrict__ start)
{
    using namespace kasa_inflate;
    __shared__ FindLds s;
    const uint32_t lane = threadIdx.x, c = blockIdx.x + 1u;
    if (c >= nChunks) return;
    const uint64_t lo = 8ull * (dataAt + (uint64_t)c * chunkBytes);
    uint64_t hi = lo + 8ull * chunkBytes;
    if (hi > 8ull * inLen) hi = 8ull * inLen;
    for (uint64_t b = lo; b < hi; b += 64u) {                         // (lo is a multiple of 8: the 64 offsets lie in 8 bytes)
        const uint64_t p = b + lane;
        unsigned long long mask = __ballot(p < hi && header_plausible(in, inLen, p));
        while (mask) {                                                // uniform: the survivors in order, one at a time
            const uint64_t q = b + (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1ull;
            __syncthreads();
            window_load(s.win, in, inLen, (uint32_t)(q >> 3), lane, 64u);
            __syncthreads();
            // (on the state in LDS, as inflate_kernel does: see there)
            if (lane == 0) { dec_at(s.d, inLen, q); s.d.reload = 0; start_skip(s.d, s.win, q); block_header(s.d, s.t, s.win); }
            __syncthreads();
            if (s.d.status == KASA_INFLATE_OK && s.d.kind == CODED) { if (lane == 0) start[c] = q; return; }
        }
    }
    if (lane == 0) start[c] = NONE;
}

struct DecodeLds {
    Tables t;
    Dec d;
    uint8_t win[WINDOW];
    uint32_t tok[QUEUE], pos[QUEUE];
    uint32_t n, skip, endSym, final;
    unsigned long long endBit;
};

// One wavefront per job: whole blocks from job.startBit until a block boundary at or behind job.stopBit, as symbols.
// Behind the capacity nothing is stored and the decoder goes on counting (Result.need).
__global__ __launch_bounds__(64) void decode_kernel(const uint8_t *__restrict__ in, uint32_t inLen, const Job *__restrict__ jobs, uint32_t nJobs, Result *__restrict__ res)
{
    using namespace kasa_inflate;
    __shared__ DecodeLds s;
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x >= nJobs) return;
    const Job job = jobs[blockIdx.x];
    uint16_t *sym = job.sym;
    const uint32_t cap = job.cap;
    if (lane == 0) { dec_at(s.d, inLen, job.startBit); s.skip = 1; s.endBit = job.startBit; s.endSym = 0; s.final = 0; }
    __syncthreads();
    int64_t fenced = 0;                                    // the job's symbols below this are written and visible to every lane
    for (;;) {
        const uint32_t st = s.d.status, kind = s.d.kind;
        if (st != KASA_INFLATE_OK || kind == DONE) break;
        if (s.d.reload || s.d.winPos >= RELOAD) {
            const uint32_t base = s.d.winBase + s.d.winPos;
            __syncthreads();
            window_load(s.win, in, inLen, base, lane, 64u);
            __syncthreads();
            if (lane == 0) {
                s.d.winBase = base; s.d.winPos = 0; s.d.reload = 0;
                if (s.skip) { start_skip(s.d, s.win, job.startBit); s.skip = 0; }
            }
            __syncthreads();
        }
        if (kind == NEED_HEADER) {
            const uint64_t at = bit_pos(s.d);
            const uint32_t outPos = s.d.outPos;
            __syncthreads();
            if (lane == 0) { s.endBit = at; s.endSym = outPos; }
            if (at >= job.stopBit) break;                  // (uniform)
            if (lane == 0) block_header(s.d, s.t, s.win);  // on the state in LDS: see inflate_kernel
            __syncthreads();
            if (s.d.status != KASA_INFLATE_OK) break;
            if (s.d.kind == STORED) {
                const uint32_t src = s.d.storedSrc, len = s.d.storedLen, to = s.d.outPos;
                if (len > MAX_JOB_SYMS - to) { __syncthreads(); if (lane == 0) s.d.status = KASA_INFLATE_SPAN; __syncthreads(); break; }
                for (uint32_t i = lane; i < len; i += 64u) if (to + i < cap) sym[to + i] = in[src + i];
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
        if (lane == 0) { Dec d = s.d; s.n = decode_symbols16(d, s.t, s.win, s.tok, s.pos, job.hist); s.d = d; }
        __syncthreads();
        const uint32_t n = s.n;
        for (uint32_t k = lane; k < n; k += 64u) { const uint32_t t = s.tok[k]; if (!(t >> 16) && s.pos[k] < cap) sym[s.pos[k]] = (uint16_t)t; }
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.tok[k]);
            const uint32_t len = t >> 16;
            if (!len) continue;
            const uint32_t dist = t & 0xFFFFu, p = (uint32_t)__builtin_amdgcn_readfirstlane((int)s.pos[k]);
            if (p >= cap) break;                           // counting only from here on
            const int64_t src = (int64_t)p - (int64_t)dist, srcEnd = dist < len ? (int64_t)p : src + (int64_t)len;
            if (srcEnd > fenced) { __syncthreads(); fenced = p; }          // (uniform: every lane has the same token)
            for (uint32_t i = lane; i < len; i += 64u) if (p + i < cap) sym[p + i] = match_symbol(sym, p, dist, i);
        }
        __syncthreads();
    }
    __syncthreads();
    if (lane == 0) {
        Result r;
        r.endBit = s.endBit; r.nSym = s.endSym; r.final = 0;
        if (s.d.status == KASA_INFLATE_OK && s.d.kind == DONE) { r.endBit = bit_pos(s.d); r.nSym = s.d.outPos; r.final = 1; }
        r.need = s.d.outPos; r.status = s.d.status; r.ranOut = ran_out(s.d) ? 1u : 0u; r.pad = 0;
        res[blockIdx.x] = r;
    }
}

// ONE workgroup: the last HIST bytes of every confirmed chunk, chunk after chunk, into the text
__global__ __launch_bounds__(CHAIN_THREADS) void chain_kernel(const Seg *__restrict__ segs, uint32_t nSegs, uint8_t *text, uint64_t total,
                                                              const uint8_t *__restrict__ prev, uint32_t prevLen,
                                                              unsigned long long *__restrict__ markers, uint32_t *__restrict__ bad)
{
    uint32_t mine = 0; bool wrong = false;
    for (uint32_t i = 0; i < nSegs; ++i) {
        const Seg g = segs[i];
        for (uint64_t k = tail_begin(g.off, g.n) + threadIdx.x; k < g.off + g.n && k < total; k += CHAIN_THREADS) {
            const uint16_t v = g.sym[k - g.off];
            mine += v >= MARK;
            text[k] = resolve(v, g.off, text, prev, prevLen, &wrong);
        }
        __syncthreads();                                   // the next chunk's markers read what this one wrote
    }
    if (mine) atomicAdd(markers, (unsigned long long)mine);
    if (wrong) atomicOr(bad, 1u);
}

// Everything below the chunks' tails: a thread takes WRITE_PER_THREAD positions a workgroup's width apart
__global__ __launch_bounds__(WRITE_THREADS) void write_kernel(const Seg *__restrict__ segs, uint32_t nSegs, uint8_t *text, uint64_t total,
                                                              const uint8_t *__restrict__ prev, uint32_t prevLen,
                                                              unsigned long long *__restrict__ markers, uint32_t *__restrict__ bad)
{
    uint32_t mine = 0; bool wrong = false;
    const uint64_t base = (uint64_t)blockIdx.x * (WRITE_THREADS * WRITE_PER_THREAD);
    for (uint32_t j = 0; j < WRITE_PER_THREAD; ++j) {
        const uint64_t k = base + (uint64_t)j * WRITE_THREADS + threadIdx.x;
        if (k >= total) break;
        uint32_t lo = 0, hi = nSegs;                       // the last chunk that begins at or before k (chunks of no text share an offset)
        while (hi - lo > 1u) { const uint32_t mid = (lo + hi) / 2u; if (segs[mid].off <= k) lo = mid; else hi = mid; }
        const Seg g = segs[lo];
        if (k - g.off >= g.n || k >= tail_begin(g.off, g.n)) continue;
        const uint16_t v = g.sym[k - g.off];
        mine += v >= MARK;
        text[k] = resolve(v, g.off, text, prev, prevLen, &wrong);         // (a marker points into a tail: the chain pass wrote it, this pass does not)
    }
    if (mine) atomicAdd(markers, (unsigned long long)mine);
    if (wrong) atomicOr(bad, 1u);
}

// CRC-32 of text[0, n): a thread takes CRC_SLICE bytes from the register `init` (the first slice) or 0, shifts the result to
// the text's end and folds it into *out.  The CRC is ~*out; *out is also the register a following span goes on from.
__global__ __launch_bounds__(CRC_THREADS) void crc_kernel(const uint8_t *__restrict__ text, uint64_t n, uint32_t init, uint32_t *__restrict__ out)
{
    __shared__ uint32_t tab[256];
    for (uint32_t i = threadIdx.x; i < 256u; i += CRC_THREADS) {
        uint32_t c = i;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kasa_bgzf::CRC_POLY : c >> 1;
        tab[i] = c;
    }
    __syncthreads();
    const uint64_t b = ((uint64_t)blockIdx.x * CRC_THREADS + threadIdx.x) * CRC_SLICE;
    if (b >= n) return;
    const uint64_t e = b + CRC_SLICE < n ? b + CRC_SLICE : n;
    uint32_t c = b ? 0u : init;
    for (uint64_t i = b; i < e; ++i) c = tab[(c ^ text[i]) & 0xFFu] ^ (c >> 8);
    // x^(8 (n - e)): the exponent modulo the group's order 2^32 - 1
    const uint32_t sh = (uint32_t)((8ull * (n - e)) % 0xFFFFFFFFull);
    atomicXor(out, kasa_bgzf::crc_mul(c, kasa_bgzf::crc_xpow(sh)));
}
#endif

} // namespace kasa_gunzip
