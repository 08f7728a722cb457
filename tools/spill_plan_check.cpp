// spill_plan_check -- the slab plan of kasa_amd/csrc/kasa_spill_plan.h (what kasa_build_finish_begin runs on the spilled runs of
// a build) compiled alone for the CPU, so that it runs under AddressSanitizer and UBSan as an ordinary program: nothing is
// preloaded.  Build: make tools/spill_plan_check.
// Usage: spill_plan_check FILE ...  A FILE holds "letters budget runs", then per run its length and its keys in ascending order, one
// hexadecimal number each (12 letters: 64-bit keys, 25 letters: 128-bit keys).  Prints per file
//     file FILE
//     heaviest PREFIX COUNT
//     slab I FIRST LAST INPUT LO:HI ...        (one line per slab, a slice per run)
//     largest INPUT
// or, instead of the slabs, "refused TEXT".  tests/test_spill_cpu.py holds the output to tests/spill_corpus.py's restatement.
#include "../kasa_amd/csrc/kasa_spill_plan.h"

#include <cinttypes>
#include <cstring>
#include <fstream>
#include <iostream>

typedef unsigned __int128 key128;

static bool parse_hex(const std::string &s, key128 &out)
{
    if (s.empty() || s.size() > 32) return false;
    out = 0;
    for (char c : s) {
        int d;
        if (c >= '0' && c <= '9') d = c - '0';
        else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
        else return false;
        out = (out << 4) | (key128)d;
    }
    return true;
}

template <class Key>
static int run(std::istream &in, int letters, uint64_t budget, size_t nRuns)
{
    std::vector<std::vector<Key>> runs(nRuns);
    for (size_t r = 0; r < nRuns; ++r) {
        uint64_t n;
        if (!(in >> n)) { fprintf(stderr, "run %zu: no length\n", r); return 2; }
        runs[r].resize((size_t)n);
        for (uint64_t i = 0; i < n; ++i) {
            std::string w;
            key128 x;
            if (!(in >> w) || !parse_hex(w, x) || (x >> (5 * letters)) != 0) { fprintf(stderr, "run %zu: bad key %" PRIu64 "\n", r, i); return 2; }
            runs[r][(size_t)i] = (Key)x;
            if (i && !(runs[r][(size_t)i - 1] <= runs[r][(size_t)i])) { fprintf(stderr, "run %zu: key %" PRIu64 " descends\n", r, i); return 2; }
        }
    }
    std::vector<const Key *> keys(nRuns);
    std::vector<uint64_t> n(nRuns);
    for (size_t r = 0; r < nRuns; ++r) { keys[r] = runs[r].data(); n[r] = runs[r].size(); }
    kasa_spill_plan::Plan plan;
    const bool ok = kasa_spill_plan::make_plan<Key>(keys.data(), n.data(), nRuns, letters, budget, plan, 1);
    for (unsigned threads : {2u, 3u, 8u}) {                            // the heaviest prefix found by several threads is the same
        kasa_spill_plan::Plan again;
        kasa_spill_plan::make_plan<Key>(keys.data(), n.data(), nRuns, letters, budget, again, threads);
        if (again.heaviestPrefix != plan.heaviestPrefix || again.heaviestCount != plan.heaviestCount || again.slabs.size() != plan.slabs.size()) {
            fprintf(stderr, "%u threads: heaviest %u %" PRIu64 ", one thread: %u %" PRIu64 "\n", threads, again.heaviestPrefix, again.heaviestCount, plan.heaviestPrefix, plan.heaviestCount);
            return 3;
        }
    }
    printf("heaviest %u %" PRIu64 "\n", plan.heaviestPrefix, plan.heaviestCount);
    if (!ok) { printf("refused %s\n", kasa_spill_plan::refusal_text(plan).c_str()); return 0; }
    for (size_t s = 0; s < plan.slabs.size(); ++s) {
        const kasa_spill_plan::Slab &sl = plan.slabs[s];
        printf("slab %zu %u %u %" PRIu64, s, sl.firstPrefix, sl.lastPrefix, sl.input);
        for (size_t r = 0; r < nRuns; ++r) printf(" %" PRIu64 ":%" PRIu64, sl.lo[r], sl.hi[r]);
        printf("\n");
    }
    printf("largest %" PRIu64 "\n", plan.largestSlab);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: spill_plan_check FILE ...\n"); return 2; }
    for (int i = 1; i < argc; ++i) {
        std::ifstream in(argv[i]);
        int letters; uint64_t budget; size_t nRuns;
        if (!(in >> letters >> budget >> nRuns) || (letters != 12 && letters != 25)) { fprintf(stderr, "%s: bad header\n", argv[i]); return 2; }
        printf("file %s\n", argv[i]);
        if (int rc = letters == 12 ? run<uint64_t>(in, letters, budget, nRuns) : run<key128>(in, letters, budget, nRuns)) return rc;
    }
    return 0;
}
