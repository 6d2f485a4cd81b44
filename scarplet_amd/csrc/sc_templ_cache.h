// Template coefficient planes kept across searches: the key of an entry and the book-keeping of budget and LRU.
//
// What the template forward chain (k_windows -> k_fwd_rows_templ -> k_fwd_cols_tsym / k_split_templ_sym) leaves behind
// - the real coefficient planes wh / mh and the per-template sums - depends on the descriptors, the axis values under
// the windows, the tile size, the chain's route and parity, and on nothing of the DEM's values.  An ENTRY is one chunk
// of sc_match_plan (one orientation run, or the nb runs a batched launch takes together: the batched column pass
// addresses the planes of a chunk as one array); its KEY is everything the chain reads, byte for byte.
//
// Nothing of HIP, so that a host compiler can build it alone: tests/templ_cache_check.cpp enumerates the key's
// properties and runs the book-keeping against stubbed allocations under AddressSanitizer / UBSan.  The device side
// (sc_api.hip) hands in an allocator and a release function and decides nothing about budget or eviction for itself.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <list>
#include <vector>
#include "../../include/scarplet_hip.h"      // sc_template

// ---- the key ------------------------------------------------------------------------------------------------
// A fixed-width hash plus the full bytes.  A hash match without equal bytes is a miss (TemplKey::equal).
struct TemplKey {
    uint64_t hash = 0;
    std::vector<unsigned char> bytes;
    bool equal(const TemplKey& o) const {
        return hash == o.hash && bytes.size() == o.bytes.size() &&
               (bytes.empty() || memcmp(bytes.data(), o.bytes.data(), bytes.size()) == 0);
    }
};

struct TemplKeyIn {
    const sc_template* t;        // the chunk's descriptors, orientation-major: nb runs of n
    int nb, n;
    double dx, dy;               // the grid spacing
    int oy, ox;                  // ny % 2, nx % 2: the DEM's parity per axis (the flip's k, the twiddles' phase table)
    int Ty, Tx;                  // the tile
    int route, parity;           // the chain's route (FftTemplFwd) and the run's flip parity (1 odd, 2 even)
    const char* build_id;        // sc_build_id(): planes of another build are never taken
    // the axis values under the chunk's windows: k_windows reads xaxis[nx/2 + qmin ..  nx/2 + qmax] and
    // yaxis[ny/2 + pmin .. ny/2 + pmax]; `xs` / `ys` are those slices over the chunk's union box.  The host layer's
    // axes are a function of (n, spacing) whose last bits move with n, so spacing and parity alone do not pin them.
    const double* xs; int nxs;
    const double* ys; int nys;
};

static_assert(sizeof(sc_template) == 120, "sc_template has no padding: its bytes are the key's");

inline uint64_t sc_templ_hash(const unsigned char* p, size_t n) {
    uint64_t h = 1469598103934665603ull;                 // FNV-1a, 64 bits
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

inline TemplKey sc_templ_key(const TemplKeyIn& in) {
    TemplKey k;
    std::vector<unsigned char>& b = k.bytes;
    auto put = [&b](const void* p, size_t n) {
        const unsigned char* c = (const unsigned char*)p;
        b.insert(b.end(), c, c + n);
    };
    const int32_t head[10] = {in.nb, in.n, in.oy, in.ox, in.Ty, in.Tx, in.route, in.parity, in.nxs, in.nys};
    put(head, sizeof(head));
    put(&in.dx, sizeof(double));
    put(&in.dy, sizeof(double));
    char id[32];
    memset(id, 0, sizeof(id));
    if (in.build_id) strncpy(id, in.build_id, sizeof(id) - 1);
    put(id, sizeof(id));
    const int nt = in.nb * in.n;
    for (int j = 0; j < nt; ++j) {
        sc_template s = in.t[j];
        s.id = 0;                        // recorded by the row pass from the current table: it does not reach the chain
        put(&s, sizeof(s));
    }
    if (in.nxs > 0) put(in.xs, sizeof(double) * (size_t)in.nxs);
    if (in.nys > 0) put(in.ys, sizeof(double) * (size_t)in.nys);
    k.hash = sc_templ_hash(b.data(), b.size());
    return k;
}

// ---- budget and LRU -----------------------------------------------------------------------------------------
struct TemplCacheStats {
    long long hits = 0, misses = 0;      // orientation runs served from an entry / sent through the chain
    long long entries = 0, bytes = 0;    // held now
    long long evictions = 0;             // entries dropped for room, for the budget, or under allocation pressure
};

struct TemplEntry {
    TemplKey key;
    void* mem = nullptr;                 // the allocator's block of `bytes`
    size_t bytes = 0;
    int runs = 0;                        // orientation runs the entry holds (the chunk's nb)
    unsigned long long epoch = 0;        // the search that last used it
};

// Rule: least recently used goes first, and a search never evicts an entry it has used itself - a search larger than
// the budget keeps what fits (the chunks it met first) and sends the rest through the chain, this time and the next;
// without that a cyclic scan would evict every entry just before its hit.
struct TemplCache {
    typedef void* (*alloc_fn)(void* user, size_t bytes);     // nullptr: no memory (the entry is not made)
    typedef void (*free_fn)(void* user, void* mem);
    alloc_fn alloc = nullptr;
    free_fn release = nullptr;
    void* user = nullptr;
    std::list<TemplEntry> lru;           // front: most recently used
    size_t budget = 0;                   // bytes; 0: off
    size_t held = 0;
    unsigned long long epoch = 0;
    TemplCacheStats st;

    void begin_search() { ++epoch; }

    TemplEntry* find(const TemplKey& k) {
        for (auto it = lru.begin(); it != lru.end(); ++it) {
            if (!it->key.equal(k)) continue;
            lru.splice(lru.begin(), lru, it);
            lru.front().epoch = epoch;
            st.hits += lru.front().runs;
            return &lru.front();
        }
        return nullptr;
    }

    void drop(std::list<TemplEntry>::iterator it) {
        if (release) release(user, it->mem);
        held -= it->bytes;
        lru.erase(it);
        ++st.evictions;
    }

    // the least recently used entry that is not `keep` and that this search has not used (`any`: that one too)
    bool drop_lru(const TemplEntry* keep, bool any) {
        for (auto it = lru.end(); it != lru.begin();) {
            --it;
            if (&*it == keep || (!any && it->epoch == epoch)) continue;
            drop(it);
            return true;
        }
        return false;
    }

    // a changed budget: entries go, least recently used first (the running search's own last), until what is held fits
    void set_budget(size_t b) {
        budget = b;
        while (held > budget && (drop_lru(nullptr, false) || drop_lru(nullptr, true))) {}
    }

    // A miss: room is made among the entries of earlier searches; nullptr where the entry does not fit the budget
    // beside what this search has used, or the allocator has no memory - the chunk then runs uncached.
    TemplEntry* insert(const TemplKey& k, size_t bytes, int runs) {
        st.misses += runs;
        if (bytes == 0 || bytes > budget) return nullptr;
        size_t pinned = 0;
        for (const TemplEntry& e : lru) if (e.epoch == epoch) pinned += e.bytes;
        if (pinned + bytes > budget) return nullptr;
        while (held + bytes > budget)
            if (!drop_lru(nullptr, false)) return nullptr;
        void* mem = alloc ? alloc(user, bytes) : nullptr;
        if (!mem) return nullptr;
        lru.emplace_front();
        TemplEntry& e = lru.front();
        e.key = k; e.mem = mem; e.bytes = bytes; e.runs = runs; e.epoch = epoch;
        held += bytes;
        return &e;
    }

    // an entry whose planes were never completed (a launch failed) must not be found again
    void discard(const TemplEntry* e) {
        for (auto it = lru.begin(); it != lru.end(); ++it)
            if (&*it == e) { drop(it); --st.evictions; return; }
    }

    void clear() {
        while (!lru.empty()) { drop(lru.begin()); --st.evictions; }
    }

    TemplCacheStats stats() const {
        TemplCacheStats s = st;
        s.entries = (long long)lru.size();
        s.bytes = (long long)held;
        return s;
    }
};
