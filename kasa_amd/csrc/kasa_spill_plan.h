// kasa_spill_plan.h -- the slab plan of a build whose runs were spilled to host memory (kasa_spill.h).  Host code only, no HIP:
// included by kasa_build.h and compiled alone, under the host's sanitizers, by tools/spill_plan_check.cpp.
//
// The runs are sorted by (k-mer, rank).  A cut between two 6-letter trie prefixes never splits a k-mer, a duplicate (k-mer,
// tax ID) pair or a trie entry, so a slab is a prefix interval, and per run the slice [lo, hi) of the keys whose prefix lies in it.
//   rule     : greedy over the distinct prefixes that occur, ascending: a slab takes whole prefixes while the sum over the runs
//              of its slice lengths (its input records) stays <= budget, and always at least one prefix
//   refusal  : a single prefix whose input records exceed the budget (the first such prefix in ascending order is named)
//   method   : bisection over the prefix values for the slab's end, one lower_bound per run and probe; 128-bit keys carry the
//              prefix in the high word, so whole keys are compared
// Beside the plan: the heaviest prefix's input records and the largest slab's input records, for kasa_build_spill_stats.  The
// heaviest prefix takes a walk over every prefix that occurs: the runs' current prefixes in a heap (more than 16 runs; fewer are
// looked at in turn), a prefix run left by a galloping search, the prefix space cut at quantiles of the longest run and walked by a few threads.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <queue>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace kasa_spill_plan {

static constexpr int PREFIX_LETTERS = 6;               // the trie's depth (RANGE_LETTERS of kasa_hip.hip)
static constexpr uint64_t PREFIX_END = 1ull << (5 * PREFIX_LETTERS);

// a spilled run in pageable host memory: keys (8 or 16 bytes each) and ranks
struct HostRun {
    void *k = nullptr;
    uint32_t *v = nullptr;
    uint64_t n = 0;
    HostRun() = default;
    HostRun(const HostRun &) = delete;
    HostRun &operator=(const HostRun &) = delete;
    HostRun(HostRun &&o) noexcept : k(o.k), v(o.v), n(o.n) { o.k = nullptr; o.v = nullptr; o.n = 0; }
    HostRun &operator=(HostRun &&o) noexcept { if (this != &o) { release(); k = o.k; v = o.v; n = o.n; o.k = nullptr; o.v = nullptr; o.n = 0; } return *this; }
    ~HostRun() { release(); }
    void release() { free(k); free(v); k = nullptr; v = nullptr; n = 0; }
};

struct Slab {
    uint32_t firstPrefix = 0, lastPrefix = 0;          // both occur in some run
    uint64_t input = 0;                                // the sum of the slice lengths
    std::vector<uint64_t> lo, hi;                      // per run
};

struct Plan {
    std::vector<Slab> slabs;
    uint64_t largestSlab = 0;                          // input records
    uint32_t heaviestPrefix = 0;
    uint64_t heaviestCount = 0;                        // input records of the heaviest prefix (the first of them, ascending)
    bool refused = false;
    uint32_t badPrefix = 0;
    uint64_t badCount = 0, budget = 0;
};

template <class Key> static inline uint32_t prefix_of(Key k, int letters) { return (uint32_t)(k >> (5 * (letters - PREFIX_LETTERS))); }

// first index in [from, n) of the run whose prefix is >= p (p <= PREFIX_END)
template <class Key> static inline uint64_t prefix_lower_bound(const Key *k, uint64_t from, uint64_t n, uint64_t p, int letters)
{
    const Key bound = (Key)p << (5 * (letters - PREFIX_LETTERS));
    return (uint64_t)(std::lower_bound(k + from, k + n, bound) - k);
}

// the same, reached from `from` in steps that double: a prefix run of length L costs O(log L)
template <class Key> static inline uint64_t prefix_gallop(const Key *k, uint64_t from, uint64_t n, uint64_t p, int letters)
{
    const Key bound = (Key)p << (5 * (letters - PREFIX_LETTERS));
    uint64_t step = 1, lo = from, hi = from;
    while (hi < n && k[hi] < bound) { lo = hi + 1; hi = n - hi > step ? hi + step : n; step <<= 1; }
    return (uint64_t)(std::lower_bound(k + lo, k + hi, bound) - k);
}

// the heaviest prefix among [pBegin, pEnd), the first of them in ascending order: all runs walked together, prefix by prefix
template <class Key>
static void heaviest_in(const Key *const *keys, const uint64_t *n, size_t nRuns, int letters, uint64_t pBegin, uint64_t pEnd, uint32_t &bestPrefix, uint64_t &bestCount)
{
    typedef std::pair<uint32_t, size_t> Item;                          // a run's current prefix, the run
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    std::vector<uint64_t> at(nRuns), end(nRuns);
    for (size_t r = 0; r < nRuns; ++r) {
        at[r] = prefix_lower_bound<Key>(keys[r], 0, n[r], pBegin, letters);
        end[r] = prefix_lower_bound<Key>(keys[r], at[r], n[r], pEnd, letters);
        if (nRuns > 16 && at[r] < end[r]) heap.push(Item(prefix_of<Key>(keys[r][at[r]], letters), r));
    }
    bestPrefix = 0; bestCount = 0;
    if (nRuns <= 16) {                                                 // few runs: the smallest current prefix by looking at all of them
        for (;;) {
            uint64_t p = PREFIX_END;
            for (size_t r = 0; r < nRuns; ++r) if (at[r] < end[r]) p = std::min<uint64_t>(p, prefix_of<Key>(keys[r][at[r]], letters));
            if (p == PREFIX_END) return;
            uint64_t cnt = 0;
            for (size_t r = 0; r < nRuns; ++r) {
                if (at[r] >= end[r] || prefix_of<Key>(keys[r][at[r]], letters) != p) continue;
                const uint64_t e = prefix_gallop<Key>(keys[r], at[r], end[r], p + 1, letters);
                cnt += e - at[r];
                at[r] = e;
            }
            if (cnt > bestCount) { bestCount = cnt; bestPrefix = (uint32_t)p; }
        }
    }
    while (!heap.empty()) {
        const uint32_t p = heap.top().first;
        uint64_t cnt = 0;
        while (!heap.empty() && heap.top().first == p) {
            const size_t r = heap.top().second;
            heap.pop();
            const uint64_t e = prefix_gallop<Key>(keys[r], at[r], end[r], (uint64_t)p + 1, letters);
            cnt += e - at[r];
            at[r] = e;
            if (e < end[r]) heap.push(Item(prefix_of<Key>(keys[r][e], letters), r));
        }
        if (cnt > bestCount) { bestCount = cnt; bestPrefix = p; }
    }
}

// The plan of `nRuns` runs (keys[r][0, n[r]) ascending) under `budget` input records per slab.  Returns false on a refusal
// (plan.refused, badPrefix, badCount), with the slabs before it in plan.slabs.  threads: for the heaviest prefix (0: one per 2^24
// records, eight at the most).
template <class Key>
static bool make_plan(const Key *const *keys, const uint64_t *n, size_t nRuns, int letters, uint64_t budget, Plan &plan, unsigned threads = 0)
{
    plan = Plan();
    plan.budget = budget;
    {
        size_t big = 0;
        uint64_t total = 0;
        for (size_t r = 0; r < nRuns; ++r) { total += n[r]; if (n[r] > n[big]) big = r; }
        if (!threads) threads = (unsigned)std::min<uint64_t>(8, 1 + (total >> 24));
        // the prefix space cut where the longest run's quantiles fall
        std::vector<uint64_t> cut(threads + 1, PREFIX_END);
        cut[0] = 0;
        for (unsigned t = 1; t < threads && nRuns && n[big]; ++t) cut[t] = std::max<uint64_t>(cut[t - 1], prefix_of<Key>(keys[big][n[big] / threads * t], letters));
        std::vector<uint32_t> bestP(threads, 0);
        std::vector<uint64_t> bestC(threads, 0);
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < threads; ++t)
            pool.emplace_back([&, t] { heaviest_in<Key>(keys, n, nRuns, letters, cut[t], cut[t + 1], bestP[t], bestC[t]); });
        heaviest_in<Key>(keys, n, nRuns, letters, cut[0], cut[1], bestP[0], bestC[0]);
        for (std::thread &th : pool) th.join();
        for (unsigned t = 0; t < threads; ++t)
            if (bestC[t] > plan.heaviestCount) { plan.heaviestCount = bestC[t]; plan.heaviestPrefix = bestP[t]; }
    }
    std::vector<uint64_t> pos(nRuns, 0), end(nRuns, 0);
    auto count_to = [&](uint64_t pEnd) {                              // input records of [the slab's start, pEnd); fills end[]
        uint64_t c = 0;
        for (size_t r = 0; r < nRuns; ++r) { end[r] = prefix_lower_bound<Key>(keys[r], pos[r], n[r], pEnd, letters); c += end[r] - pos[r]; }
        return c;
    };
    for (;;) {
        uint64_t first = PREFIX_END;
        for (size_t r = 0; r < nRuns; ++r) if (pos[r] < n[r]) first = std::min<uint64_t>(first, prefix_of<Key>(keys[r][pos[r]], letters));
        if (first == PREFIX_END) break;
        uint64_t lo = first + 1, hi = PREFIX_END;                     // the slab ends before prefix `lo` at least, `hi` at most
        const uint64_t one = count_to(lo);
        if (one > budget) { plan.refused = true; plan.badPrefix = (uint32_t)first; plan.badCount = one; return false; }
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (count_to(mid) <= budget) lo = mid; else hi = mid - 1;
        }
        Slab s;
        s.input = count_to(lo);
        s.firstPrefix = (uint32_t)first;
        s.lo = pos; s.hi = end;
        for (size_t r = 0; r < nRuns; ++r) if (end[r] > pos[r]) s.lastPrefix = std::max(s.lastPrefix, prefix_of<Key>(keys[r][end[r] - 1], letters));
        plan.largestSlab = std::max(plan.largestSlab, s.input);
        plan.slabs.push_back(std::move(s));
        pos = end;
    }
    return true;
}

// the text of a refusal, without the caller's name in front
static inline std::string refusal_text(const Plan &plan)
{
    char buf[256];
    snprintf(buf, sizeof(buf), "prefix %u alone brings %llu input records to a slab, the resident budget is %llu records", plan.badPrefix,
             (unsigned long long)plan.badCount, (unsigned long long)plan.budget);
    return buf;
}

} // namespace kasa_spill_plan
