// The reference of tests/rank_corpus.py: std::sort itself over the hits of a read, with the comparator and the tuple type of
// Compare::scoringFunc (Compare.hpp:1582; the same as tests/stdsort_check.cpp), and what kasa_amd/csrc/stdsort_order.h (host
// mode) says about the same row.  tests/test_rank_corpus_cpu.py and tests/test_gpu_rank_corpus.py compile and run this.
//
//   rank_reference <in> <out> <need>
// in:  uint64 nRows, uint64 off[nRows + 1], uint32 tax[nnz], float score[nnz], double rel[nnz]   (the kept hits of every
//      row, taxon strictly ascending within a row; nnz = off[nRows]; rows of fewer than 65 536 hits)
// out: uint32 order[nnz]     order[off[r] + k] = position within row r of the hit std::sort leaves at place k
//      uint8  heap[nRows]    stdsort_order gives up on the whole row (libstdc++ heap-sorts a range of it)
//      uint8  short[nRows]   stdsort_order gives up even when only the first <need> places are asked for
//      uint32 covered[nRows] the leading places the <need>-only sort made final (where it did not give up)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>
#include "../kasa_amd/csrc/stdsort_order.h"

template <class T> static bool get_n(std::FILE *f, std::vector<T> &v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }
template <class T> static bool put_n(std::FILE *f, const std::vector<T> &v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc != 4) { std::fprintf(stderr, "usage: rank_reference <in> <out> <need>\n"); return 2; }
    const int need = std::atoi(argv[3]);
    std::FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::perror(argv[1]); return 2; }
    uint64_t nRows = 0;
    std::vector<uint64_t> off; std::vector<uint32_t> tax; std::vector<float> score; std::vector<double> rel;
    if (std::fread(&nRows, 8, 1, in) != 1 || !get_n(in, off, (size_t)nRows + 1) || off[0] != 0) { std::fprintf(stderr, "short input\n"); return 2; }
    for (uint64_t r = 0; r < nRows; ++r) if (off[r + 1] < off[r] || off[r + 1] - off[r] >= 65536) { std::fprintf(stderr, "bad row %llu\n", (unsigned long long)r); return 2; }
    const size_t nnz = (size_t)off[nRows];
    if (!get_n(in, tax, nnz) || !get_n(in, score, nnz) || !get_n(in, rel, nnz)) { std::fprintf(stderr, "short input\n"); return 2; }
    std::fclose(in);
    std::vector<uint32_t> order(nnz), covered((size_t)nRows);
    std::vector<uint8_t> heap((size_t)nRows), shrt((size_t)nRows);
    typedef std::tuple<size_t, float, double> Hit;                  // what Compare::scoringFunc sorts: (taxon, score, relative score)
    std::vector<Hit> res;
    std::vector<uint16_t> ids;
    for (uint64_t r = 0; r < nRows; ++r) {
        const size_t lo = (size_t)off[r];
        const int n = (int)(off[r + 1] - off[r]);
        res.resize((size_t)n);
        for (int i = 0; i < n; ++i) {
            if (i && tax[lo + i] <= tax[lo + i - 1]) { std::fprintf(stderr, "row %llu: taxa do not ascend\n", (unsigned long long)r); return 2; }
            res[(size_t)i] = std::make_tuple((size_t)tax[lo + i], score[lo + i], rel[lo + i]);
        }
        std::sort(res.begin(), res.end(), [](const Hit &a, const Hit &b) { return std::get<2>(a) > std::get<2>(b); });
        for (int k = 0; k < n; ++k)
            order[lo + k] = (uint32_t)(std::lower_bound(tax.begin() + lo, tax.begin() + lo + n, (uint32_t)std::get<0>(res[(size_t)k])) - (tax.begin() + lo));
        const double *rl = rel.data() + lo;
        auto less = [rl](uint16_t x, uint16_t y) { return rl[x] > rl[y]; };
        ids.resize((size_t)n);
        for (int i = 0; i < n; ++i) ids[(size_t)i] = (uint16_t)i;
        const bool whole = stdsort_order(ids.data(), n, less);
        heap[(size_t)r] = whole ? 0 : 1;
        if (whole)                                                  // (the restatement against the real thing, on every row of the corpus)
            for (int k = 0; k < n; ++k)
                if (ids[(size_t)k] != order[lo + k]) { std::fprintf(stderr, "row %llu: stdsort_order differs from std::sort at %d\n", (unsigned long long)r, k); return 1; }
        for (int i = 0; i < n; ++i) ids[(size_t)i] = (uint16_t)i;
        int cov = 0;
        const bool first = stdsort_order(ids.data(), n, less, need, &cov);
        shrt[(size_t)r] = first ? 0 : 1;
        covered[(size_t)r] = first ? (uint32_t)cov : 0u;
        if (first)
            for (int k = 0; k < cov; ++k)
                if (ids[(size_t)k] != order[lo + k]) { std::fprintf(stderr, "row %llu: the prefix of stdsort_order differs from std::sort at %d\n", (unsigned long long)r, k); return 1; }
    }
    std::FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    const bool ok = put_n(out, order) && put_n(out, heap) && put_n(out, shrt) && put_n(out, covered);
    return std::fclose(out) == 0 && ok ? 0 : 2;
}
