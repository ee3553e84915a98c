// dsq_plugin_pool.h — the bookkeeping of the plug-in device cache (dsq_plugin_cache.h): resident matrices under an LRU byte
// budget and a size-matched free list of device buffers.  Host code only, no HIP: device memory comes through the two function
// pointers of Cache (hipMalloc / hipFree in dsq_capi_inf.hip, a fake allocator in tests/hostsim).
//
// An Entry* obtained from find() or insert() stays valid until the next begin_call(): entries never move (a std::list), and
// the only evictions inside a call (take(), insert()) spare the entries that call has touched.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <iterator>
#include <list>
#include <utility>
#include <vector>

namespace dsq_pc {

struct Digest {
    uint64_t a = 0, b = 0;
};
inline bool operator==(const Digest& x, const Digest& y) { return x.a == y.a && x.b == y.b; }

enum Kind { kCounts = 0, kF64 = 1 };

struct Entry {
    int kind = 0, N = 0, G = 0, ld = 0;
    Digest dg;
    void* d = nullptr;
    size_t cap = 0;
    uint64_t tick = 0;
    int positive = -1;  // fp64 matrices: every element positive, finite, normal?  -1: not checked yet
    // counts: gene lists of the mixed-design dispersion kernel (genes with a count beyond its 16-bit staging stay on the
    // general kernel), built on first use (attach_lists)
    int n_rows = 0, n_waves = 0;
    void* d_lists = nullptr;
    size_t lists_cap = 0;
};

struct Stats {
    uint64_t hits = 0, misses = 0, adopted = 0, evictions = 0, h2d_bytes = 0, d2h_bytes = 0, mallocs = 0, verified = 0;
    double hash_ms = 0.0;
};

struct Cache {
    bool (*alloc)(void** p, size_t bytes) = nullptr;  // device memory: false when there is none
    void (*free)(void* p) = nullptr;
    bool enabled = true;
    bool verify = false;  // DSQ_PLUGIN_CACHE_VERIFY: a hit is re-uploaded and compared with the resident copy
    size_t budget = 0, resident = 0, pooled = 0;
    uint64_t tick = 0, call_tick = 0;
    int hash_threads = 32;
    std::list<Entry> ents;
    std::vector<std::pair<size_t, void*>> free_bufs;
    unsigned long long* d_acc = nullptr;  // 4 x u64 on the device: digest a, b, flag, spare
    unsigned long long* h_acc = nullptr;  // page-locked mirror
    Stats st;
};

// the least recently used of `l` (elements with a `tick`) among those last used at or before `upto`; end() if there is none
template <class L>
typename L::iterator lru(L& l, uint64_t upto = UINT64_MAX) {
    auto best = l.end();
    for (auto it = l.begin(); it != l.end(); ++it)
        if (it->tick <= upto && (best == l.end() || it->tick < best->tick)) best = it;
    return best;
}

inline void give(Cache& c, void* p, size_t cap) {
    if (p == nullptr) return;
    c.free_bufs.emplace_back(cap, p);
    c.pooled += cap;
    // free list and resident matrices share ONE budget (a context used to be able to pin twice the budget: the cache plus
    // as much again on the free list); the free list keeps what the resident matrices leave of it
    while (c.pooled + c.resident > c.budget && !c.free_bufs.empty()) {
        const auto big = std::max_element(c.free_bufs.begin(), c.free_bufs.end(),
                                          [](const auto& x, const auto& y) { return x.first < y.first; });
        c.free(big->second);  // (hipFree synchronises the device: rare)
        c.pooled -= big->first;
        c.free_bufs.erase(big);
    }
}

// an entry's buffers go to the free list (to_pool) or straight back to the allocator
inline void drop(Cache& c, std::list<Entry>::iterator it, bool to_pool) {
    c.resident -= it->cap + it->lists_cap;
    if (to_pool) {
        give(c, it->d, it->cap);
        give(c, it->d_lists, it->lists_cap);
    } else {
        c.free(it->d);
        if (it->d_lists) c.free(it->d_lists);
    }
    c.ents.erase(it);
}

inline void free_pool(Cache& c) {
    for (auto& f : c.free_bufs) c.free(f.second);
    c.free_bufs.clear();
    c.pooled = 0;
}

inline bool take(Cache& c, size_t bytes, void** p, size_t* cap) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    int best = -1;
    for (int i = 0; i < (int)c.free_bufs.size(); ++i) {
        const size_t k = c.free_bufs[(size_t)i].first;
        if (k >= bytes && k <= 2 * bytes + 4096 && (best < 0 || k < c.free_bufs[(size_t)best].first)) best = i;
    }
    if (best >= 0) {
        *cap = c.free_bufs[(size_t)best].first;
        *p = c.free_bufs[(size_t)best].second;
        c.pooled -= *cap;
        c.free_bufs.erase(c.free_bufs.begin() + best);
        return true;
    }
    bool ok = c.alloc(p, bytes);
    if (!ok) {  // out of memory: drop the free list and retry ...
        free_pool(c);
        ok = c.alloc(p, bytes);
    }
    while (!ok) {  // ... then the resident matrices the running call has not touched, least recently used first (their
                   // buffers must go back to the allocator: on the free list they would still hold the memory)
        const auto v = lru(c.ents, c.call_tick);
        if (v == c.ents.end()) break;
        drop(c, v, false);
        ++c.st.evictions;
        ok = c.alloc(p, bytes);
    }
    if (ok) {
        *cap = bytes;
        ++c.st.mallocs;
    }
    return ok;
}

inline Entry* find(Cache& c, int kind, int N, int G, const Digest& dg) {
    for (Entry& e : c.ents)
        if (e.kind == kind && e.N == N && e.G == G && e.dg == dg) {
            e.tick = ++c.tick;
            return &e;
        }
    return nullptr;
}

// a new resident matrix; least-recently-used entries that the running call has not touched make room
inline Entry* insert(Cache& c, const Entry& e) {
    while (c.resident + e.cap > c.budget) {
        const auto v = lru(c.ents, c.call_tick);
        if (v == c.ents.end()) break;  // everything resident belongs to this call: over budget until it ends
        drop(c, v, true);
        ++c.st.evictions;
    }
    c.resident += e.cap;
    c.ents.push_back(e);
    c.ents.back().tick = ++c.tick;
    return &c.ents.back();
}

// the mixed-design gene lists of a resident count matrix (a buffer from take()) are the entry's from here on
inline void attach_lists(Cache& c, Entry* e, void* p, size_t cap) {
    e->d_lists = p;
    e->lists_cap = cap;
    c.resident += cap;
}

// start of an Inference-level call: entries touched from here on are not evicted by it; with the cache switched off
// (or a budget the last call overran) what the previous call left goes back to the free list
inline void begin_call(Cache& c) {
    c.call_tick = c.tick;
    if (!c.enabled) {
        while (!c.ents.empty()) drop(c, std::prev(c.ents.end()), true);
    } else {
        while (c.resident > c.budget && !c.ents.empty()) {
            drop(c, lru(c.ents), true);
            ++c.st.evictions;
        }
    }
}

inline void clear(Cache& c) {
    while (!c.ents.empty()) drop(c, std::prev(c.ents.end()), true);
    free_pool(c);
}

}  // namespace dsq_pc
