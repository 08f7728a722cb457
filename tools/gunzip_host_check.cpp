// gunzip_host_check -- the bodies of kasa_amd/csrc/kasa_gunzip.h (header validation, the 16-bit symbol decoder, the window
// resolve and the marker replacement) and its rounds (inflate_file / inflate_stream, the very template the device runs)
// compiled for the CPU and run under AddressSanitizer + UBSan over a directory of gzip files:
//   NAME.gz      a gzip file: one or more members, none of them BGZF
//   NAME.raw     the text it has to inflate to, or
//   NAME.status  "<KASA_INFLATE_* code> <member index>": the file has to be rejected with exactly that
// The stream, every job's symbols and the text live in heap blocks of exactly their size, so a load behind the stream or a
// store behind a capacity is an error of the sanitizer and not a silent pass.  Build: make tools/gunzip_host_check.
// Usage: gunzip_host_check DIR [chunkBytes ...]   (default: 64 256 1024 0; 0 is the library's default)
//   -> per file and chunk size one line with the chunk statistics kasa_gzip_inflate gives in stats8:
//        NAME @64: status 0, 1234 bytes; chunks 20 started 9 confirmed 9 rejected 0 rounds 1 markers 77 reruns 0 members 1
//      exit code 0 when every file gave what its companion says at every chunk size.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <dirent.h>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>

#include "../kasa_amd/csrc/kasa_gunzip.h"

static bool slurp(const std::string &path, std::vector<uint8_t> &out)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

struct HostBackend {
    const uint8_t *in;
    uint32_t nBytes;
    uint8_t *text;
    uint64_t textCap;
    std::vector<std::unique_ptr<uint16_t[]>> syms;

    void begin() { syms.clear(); }
    int find(uint64_t dataAt, uint32_t chunkBytes, uint32_t nChunks, std::vector<uint64_t> &start)
    {
        for (uint32_t c = 1; c < nChunks; ++c) {
            const uint64_t lo = 8 * (dataAt + (uint64_t)c * chunkBytes);
            start[c] = kasa_gunzip::find_serial(in, nBytes, lo, std::min<uint64_t>(lo + 8ull * chunkBytes, 8ull * nBytes));
        }
        return KASA_OK;
    }
    int symbols(uint32_t n, uint16_t **p)
    {
        syms.emplace_back(new uint16_t[n ? n : 1]);
        *p = syms.back().get();
        return KASA_OK;
    }
    int decode(const std::vector<kasa_gunzip::Job> &js, std::vector<kasa_gunzip::Result> &rs)
    {
        for (size_t i = 0; i < js.size(); ++i) kasa_gunzip::decode_serial(in, nBytes, js[i], rs[i]);
        return KASA_OK;
    }
    int place(const std::vector<kasa_gunzip::Seg> &sg, uint64_t textAt, uint64_t total, uint64_t *markers, bool *bad)
    {
        if (textAt > textCap || total > textCap - textAt) return KASA_E_ARG;
        kasa_gunzip::place_serial(sg.data(), (uint32_t)sg.size(), text + textAt, nullptr, 0, markers, bad);
        return KASA_OK;
    }
    int crc(uint64_t textAt, uint64_t n, uint32_t *out)
    {
        uint32_t c = 0xFFFFFFFFu;
        for (uint64_t i = 0; i < n; ++i) {
            c ^= text[textAt + i];
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        }
        *out = ~c;
        return KASA_OK;
    }
};

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s DIR [chunkBytes ...]\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    std::vector<uint32_t> sizes;
    for (int i = 2; i < argc; ++i) sizes.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
    if (sizes.empty()) sizes = {64u, 256u, 1024u, 0u};
    std::vector<std::string> names;
    if (DIR *d = opendir(dir.c_str())) {
        while (dirent *e = readdir(d)) {
            const std::string f = e->d_name;
            if (f.size() > 3 && f.compare(f.size() - 3, 3, ".gz") == 0) names.push_back(f.substr(0, f.size() - 3));
        }
        closedir(d);
    } else { fprintf(stderr, "%s: cannot be listed\n", dir.c_str()); return 2; }
    std::sort(names.begin(), names.end());
    int bad = 0, runs = 0;
    for (const std::string &name : names) {
        std::vector<uint8_t> file, want, st;
        if (!slurp(dir + "/" + name + ".gz", file)) { printf("%s: unreadable\n", name.c_str()); ++bad; continue; }
        const bool hasStatus = slurp(dir + "/" + name + ".status", st), hasRaw = !hasStatus && slurp(dir + "/" + name + ".raw", want);
        if (!hasStatus && !hasRaw) { printf("%s: neither .raw nor .status\n", name.c_str()); ++bad; continue; }
        int wantCode = 0; unsigned long long wantMember = 0;
        if (hasStatus && sscanf(std::string(st.begin(), st.end()).c_str(), "%d %llu", &wantCode, &wantMember) != 2) { printf("%s: .status unreadable\n", name.c_str()); ++bad; continue; }
        std::unique_ptr<uint8_t[]> in(new uint8_t[file.size() ? file.size() : 1]);
        std::copy(file.begin(), file.end(), in.get());
        for (uint32_t chunk : sizes) {
            const uint64_t cap = hasRaw ? want.size() : (1u << 22);
            std::unique_ptr<uint8_t[]> text(new uint8_t[cap ? cap : 1]);
            HostBackend be;
            be.in = in.get(); be.nBytes = (uint32_t)file.size(); be.text = text.get(); be.textCap = cap;
            kasa_gunzip::Stats s;
            std::memset(&s, 0, sizeof s);
            int status = 0; uint64_t member = 0, nText = 0;
            const int rc = kasa_gunzip::inflate_file(be, in.get(), file.size(), chunk ? chunk : kasa_gunzip::DEFAULT_CHUNK, cap, s, &status, &member, &nText);
            bool ok = rc == KASA_OK;
            if (ok && hasStatus) ok = status == wantCode && member == wantMember;
            if (ok && hasRaw) ok = status == KASA_INFLATE_OK && nText == want.size() && std::equal(want.begin(), want.end(), text.get());
            printf("%s @%u: status %d, %llu bytes; chunks %llu started %llu confirmed %llu rejected %llu rounds %llu markers %llu reruns %llu members %llu%s\n", name.c_str(), chunk, status,
                   (unsigned long long)nText, (unsigned long long)s.chunks, (unsigned long long)s.withStart, (unsigned long long)s.confirmed, (unsigned long long)s.rejected,
                   (unsigned long long)s.rounds, (unsigned long long)s.markers, (unsigned long long)s.reruns, (unsigned long long)s.members, ok ? "" : "  MISMATCH");
            if (!ok) { printf("  rc %d, member %llu; wanted: %s\n", rc, (unsigned long long)member, hasStatus ? std::string(st.begin(), st.end()).c_str() : "the text"); ++bad; }
            ++runs;
        }
    }
    printf("%zu files, %d runs, %d wrong\n", names.size(), runs, bad);
    return bad || names.empty() ? 1 : 0;
}
