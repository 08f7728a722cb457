// inflate_host_check -- the decoder body of kasa_amd/csrc/kasa_inflate.h (bit reader, table builder, block-header parser,
// symbol loop with its validation) compiled for the CPU and run under AddressSanitizer + UBSan over a directory of BGZF spans:
//   NAME.bgzf    a span of members (it may end inside one)
//   NAME.raw     the text the span has to inflate to, or
//   NAME.status  "<KASA_INFLATE_* code> <member index>": the span has to be rejected with exactly that
// Every member's payload and output live in heap blocks of exactly their size, so a load behind the payload or a store
// behind ISIZE is an error of the sanitizer and not a silent pass.  Build: make tools/inflate_host_check.
// Usage: inflate_host_check DIR  -> one line per span, exit code 0 when every span gave what its file says.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <dirent.h>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>

#include "../kasa_amd/csrc/kasa_inflate.h"

static bool slurp(const std::string &path, std::vector<uint8_t> &out)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

static uint32_t crc32_bytes(const uint8_t *p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

// what kasa_bgzf_inflate answers for the span: status, member, text
static void inflate_span(const std::vector<uint8_t> &span, int &status, uint64_t &member, std::vector<uint8_t> &text)
{
    using namespace kasa_inflate;
    std::vector<Member> tab;
    uint64_t consumed = 0, nText = 0;
    status = walk_members(span.data(), span.size(), tab, &consumed, &nText);
    member = tab.size();
    if (status == KASA_INFLATE_OK && consumed != span.size()) status = KASA_INFLATE_CUT;
    if (status != KASA_INFLATE_OK) return;
    text.clear();
    for (size_t i = 0; i < tab.size(); ++i) {
        const Member &m = tab[i];
        std::unique_ptr<uint8_t[]> in(new uint8_t[m.payLen ? m.payLen : 1]), out(new uint8_t[m.isize ? m.isize : 1]);
        std::copy(span.begin() + (ptrdiff_t)m.payload, span.begin() + (ptrdiff_t)(m.payload + m.payLen), in.get());
        int st = inflate_member_serial(in.get(), m.payLen, out.get(), m.isize);
        if (st == KASA_INFLATE_OK && crc32_bytes(out.get(), m.isize) != m.crc) st = KASA_INFLATE_CRC;
        if (st != KASA_INFLATE_OK) { status = st; member = i; text.clear(); return; }
        text.insert(text.end(), out.get(), out.get() + m.isize);
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    std::vector<std::string> names;
    if (DIR *d = opendir(dir.c_str())) {
        while (dirent *e = readdir(d)) {
            const std::string f = e->d_name;
            if (f.size() > 5 && f.compare(f.size() - 5, 5, ".bgzf") == 0) names.push_back(f.substr(0, f.size() - 5));
        }
        closedir(d);
    } else { fprintf(stderr, "%s: cannot be listed\n", dir.c_str()); return 2; }
    std::sort(names.begin(), names.end());
    int bad = 0;
    for (const std::string &name : names) {
        std::vector<uint8_t> span, want, text;
        if (!slurp(dir + "/" + name + ".bgzf", span)) { printf("%s: unreadable\n", name.c_str()); ++bad; continue; }
        int status = 0; uint64_t member = 0;
        inflate_span(span, status, member, text);
        std::vector<uint8_t> st;
        if (slurp(dir + "/" + name + ".status", st)) {
            const std::string line(st.begin(), st.end());
            int wantCode = -1; unsigned long long wantMember = 0;
            const bool ok = sscanf(line.c_str(), "%d %llu", &wantCode, &wantMember) == 2 && status == wantCode && member == wantMember;
            printf("%s: status %d (%s) in member %llu%s\n", name.c_str(), status, status ? "rejected" : "inflated", (unsigned long long)member, ok ? "" : "  MISMATCH");
            if (!ok) { printf("  wanted: %s\n", line.c_str()); ++bad; }
        } else if (slurp(dir + "/" + name + ".raw", want)) {
            const bool ok = status == KASA_INFLATE_OK && text == want;
            printf("%s: status %d, %zu bytes%s\n", name.c_str(), status, text.size(), ok ? "" : "  MISMATCH");
            if (!ok) { if (status) printf("  member %llu\n", (unsigned long long)member); ++bad; }
        } else { printf("%s: neither .raw nor .status\n", name.c_str()); ++bad; }
    }
    printf("%zu spans, %d wrong\n", names.size(), bad);
    return bad || names.empty() ? 1 : 0;
}
