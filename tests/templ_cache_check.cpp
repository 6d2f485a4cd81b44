// The template cache's key and its book-keeping of budget and LRU (scarplet_amd/csrc/sc_templ_cache.h) on the host:
// g++ -std=c++17 -fsanitize=address,undefined, a program of its own (tests/test_templ_cache_host.py builds and runs it).
// The device allocations are stubbed out: malloc / free behind the cache's two callbacks, counted and checked.
//   * equal chunks give equal keys; every single field that reaches the template forward chain, changed alone, gives
//     another key; the id does not; a forged hash without the bytes is no match
//   * under a budget of k entries, seeded access sequences leave the entries a restated LRU list predicts (one access
//     per search, so that nothing is pinned), the hits and the misses with them
//   * a search never evicts what it has used itself: a cyclic scan larger than the budget keeps its first k chunks
//   * no entry is ever larger than the budget, what is held never exceeds it, every block is released exactly once
#include "../scarplet_amd/csrc/sc_templ_cache.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

static long long n_checked = 0, n_failed = 0;
static void fail(const char* what, int line) {
    if (n_failed++ < 20) std::fprintf(stderr, "FAIL %s (line %d)\n", what, line);
}
#define CHECK(cond) do { ++n_checked; if (!(cond)) fail(#cond, __LINE__); } while (0)

struct Rng {
    unsigned long long s;
    unsigned long long next() {
        unsigned long long z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int below(int n) { return (int)(next() % (unsigned long long)n); }
};

// ---- the stubbed device: blocks alive, bytes alive, the largest request ----
struct Device {
    std::set<void*> alive;
    size_t bytes = 0, largest = 0, cap = (size_t)-1;
    long long allocs = 0, frees = 0, bad_frees = 0;
    std::vector<std::pair<void*, size_t>> sizes;
};
static void* dev_alloc(void* user, size_t bytes) {
    Device* d = (Device*)user;
    if (d->bytes + bytes > d->cap) return nullptr;           // "out of memory"
    void* p = std::malloc(16);
    d->alive.insert(p);
    d->sizes.push_back({p, bytes});
    d->bytes += bytes;
    d->largest = std::max(d->largest, bytes);
    ++d->allocs;
    return p;
}
static void dev_free(void* user, void* mem) {
    Device* d = (Device*)user;
    if (!d->alive.erase(mem)) { ++d->bad_frees; return; }
    for (auto& s : d->sizes)
        if (s.first == mem) { d->bytes -= s.second; s.first = nullptr; break; }
    std::free(mem);
    ++d->frees;
}
static void attach(TemplCache& c, Device& d) { c.alloc = dev_alloc; c.release = dev_free; c.user = &d; }

// ---- a chunk: nb runs of n templates, and the rest of the key's input ----
struct Chunk {
    std::vector<sc_template> t;
    std::vector<double> xs, ys;
    TemplKeyIn in;
};
static Chunk make_chunk(int nb, int n, unsigned seed) {
    Chunk c;
    Rng g{seed};
    for (int b = 0; b < nb; ++b)
        for (int j = 0; j < n; ++j) {
            sc_template s;
            std::memset(&s, 0, sizeof(s));
            s.kind = SC_KIND_SCARP; s.flags = SC_FLAG_NEGATE;
            const double a = 0.1 * b + 0.01 * g.below(5);
            s.cos_a = std::cos(a); s.sin_a = std::sin(a);
            s.c = 40.0; s.d = 200.0;
            s.p0 = 2.0 * std::pow(10.0 + j, 1.5) * std::sqrt(3.141592653589793); s.p1 = 4.0 * (10.0 + j);   // one age
            s.cc = s.cos_a * s.cos_a; s.sc2 = 2.0 * s.sin_a * s.cos_a; s.ss = s.sin_a * s.sin_a;
            s.ilo = 3; s.ihi = 500; s.jlo = 3; s.jhi = 600;
            s.pmin = -20; s.pmax = 19; s.qmin = -30; s.qmax = 29;
            s.id = (uint32_t)(b * n + j);
            s.window = -1;
            c.t.push_back(s);
        }
    for (int i = 0; i < 60; ++i) c.xs.push_back(0.5 * (i - 29.5));
    for (int i = 0; i < 40; ++i) c.ys.push_back(0.5 * (i - 19.5));
    std::memset(&c.in, 0, sizeof(c.in));
    c.in.nb = nb; c.in.n = n; c.in.dx = 0.5; c.in.dy = 0.5; c.in.oy = 0; c.in.ox = 0; c.in.Ty = 512; c.in.Tx = 1024;
    c.in.route = 2; c.in.parity = 1; c.in.build_id = "0123456789abcdef";
    return c;
}
static TemplKey key_of(Chunk& c) {
    c.in.t = c.t.data();
    c.in.xs = c.xs.data(); c.in.nxs = (int)c.xs.size();
    c.in.ys = c.ys.data(); c.in.nys = (int)c.ys.size();
    return sc_templ_key(c.in);
}

static void check_keys() {
    Chunk a = make_chunk(2, 3, 7), b = make_chunk(2, 3, 7);
    const TemplKey ka = key_of(a);
    CHECK(ka.equal(key_of(b)));                              // equal chunks, equal keys (other storage)
    CHECK(ka.hash == key_of(b).hash && !ka.bytes.empty());
    // the id does not reach the chain
    for (auto& s : b.t) s.id += 1000;
    CHECK(ka.equal(key_of(b)));
    // every field that does, changed alone
    int n_fields = 0;
    auto differs = [&](auto change) {
        Chunk c = make_chunk(2, 3, 7);
        change(c);
        const TemplKey kc = key_of(c);
        CHECK(!ka.equal(kc));
        CHECK(ka.bytes != kc.bytes);                         // (the full compare alone tells them apart)
        ++n_fields;
    };
    differs([](Chunk& c) { c.in.dx = 0.25; });
    differs([](Chunk& c) { c.in.dy = 0.25; });
    differs([](Chunk& c) { c.in.oy = 1; });
    differs([](Chunk& c) { c.in.ox = 1; });
    differs([](Chunk& c) { c.in.Ty = 1024; });
    differs([](Chunk& c) { c.in.Tx = 2048; });
    differs([](Chunk& c) { c.in.route = 1; });
    differs([](Chunk& c) { c.in.parity = 2; });
    differs([](Chunk& c) { c.in.build_id = "0123456789abcdee"; });
    differs([](Chunk& c) { c.t[4].p0 *= 1.5; c.t[4].p1 *= 1.5; });                       // one age
    differs([](Chunk& c) { c.t[4].p1 = std::nextafter(c.t[4].p1, 1e300); });             //   ... by one bit
    differs([](Chunk& c) { c.t[1].cos_a = std::cos(0.5); c.t[1].sin_a = std::sin(0.5); }); // one angle
    differs([](Chunk& c) { c.t[0].cc = std::nextafter(c.t[0].cc, 2.0); });
    differs([](Chunk& c) { c.t[2].kind = SC_KIND_RICKER; });                             // kind
    differs([](Chunk& c) { c.t[2].flags = 0; });
    differs([](Chunk& c) { c.t[3].c = 80.0; });                                          // scale: the window's half-widths
    differs([](Chunk& c) { c.t[3].d = 400.0; });
    differs([](Chunk& c) { c.t[5].pmin -= 1; });                                         //   ... and its box
    differs([](Chunk& c) { c.t[5].qmax += 1; });
    differs([](Chunk& c) { c.t[0].jhi = 601; });
    differs([](Chunk& c) { c.xs[17] = std::nextafter(c.xs[17], 1e300); });               // an axis value under the windows
    differs([](Chunk& c) { c.ys[39] = std::nextafter(c.ys[39], 1e300); });
    differs([](Chunk& c) { c.xs.push_back(15.5); });
    differs([](Chunk& c) { std::swap(c.t[0], c.t[1]); });                                // the order of the templates
    CHECK(n_fields == 24);
    // the shape of the batch is part of the key: 2 x 3 and 3 x 2 of the same six descriptors
    {
        Chunk c = make_chunk(2, 3, 7);
        c.in.nb = 3; c.in.n = 2;
        CHECK(!ka.equal(key_of(c)));
    }
    // a hash match without an equal full key is a miss
    {
        Chunk c = make_chunk(2, 3, 7);
        c.in.dx = 0.25;
        TemplKey forged = key_of(c);
        forged.hash = ka.hash;
        CHECK(!ka.equal(forged));
        Device d;
        TemplCache cache;
        attach(cache, d);
        cache.set_budget(1000);
        cache.begin_search();
        CHECK(cache.insert(ka, 100, 2) != nullptr);
        CHECK(cache.find(forged) == nullptr);
        CHECK(cache.find(ka) != nullptr);
        cache.clear();
        CHECK(d.alive.empty());
    }
}

// what holds after every step
static void check_invariants(const TemplCache& c, const Device& d) {
    size_t sum = 0;
    for (const TemplEntry& e : c.lru) {
        sum += e.bytes;
        CHECK(e.bytes <= c.budget);                          // no entry larger than the budget
        CHECK(d.alive.count(e.mem) == 1);
    }
    CHECK(sum == c.held && c.held <= c.budget);
    CHECK(d.bytes == c.held && d.alive.size() == c.lru.size());
    CHECK(d.bad_frees == 0);
    const TemplCacheStats s = c.stats();
    CHECK(s.entries == (long long)c.lru.size() && s.bytes == (long long)c.held);
}

// Seeded access sequences, one access per search, entries of one size: the cache against a restated LRU list
static void check_lru(int k, int n_keys, unsigned seed) {
    Device d;
    TemplCache cache;
    attach(cache, d);
    const size_t B = 1000;
    cache.set_budget(k * B + B / 2);                         // room for k entries
    std::vector<Chunk> chunks;
    std::vector<TemplKey> keys;
    for (int i = 0; i < n_keys; ++i) {
        chunks.push_back(make_chunk(1, 2, 100 + i));
        chunks.back().in.dx = 1.0 + i;
        keys.push_back(key_of(chunks.back()));
    }
    std::vector<int> model;                                  // front: most recently used
    long long hits = 0, misses = 0, evictions = 0;
    Rng g{seed};
    for (int step = 0; step < 400; ++step) {
        const int i = g.below(n_keys);
        cache.begin_search();
        TemplEntry* e = cache.find(keys[i]);
        auto it = std::find(model.begin(), model.end(), i);
        CHECK((e != nullptr) == (it != model.end()));
        if (it != model.end()) {
            model.erase(it);
            ++hits;
        } else {
            e = cache.insert(keys[i], B, 1);
            CHECK(e != nullptr);
            ++misses;
            if ((int)model.size() == k) { model.pop_back(); ++evictions; }
        }
        model.insert(model.begin(), i);
        // the same entries in the same order
        CHECK(cache.lru.size() == model.size());
        size_t m = 0;
        for (const TemplEntry& en : cache.lru) {
            if (m < model.size()) CHECK(en.key.equal(keys[model[m]]));
            ++m;
        }
        check_invariants(cache, d);
    }
    const TemplCacheStats s = cache.stats();
    CHECK(s.hits == hits && s.misses == misses && s.evictions == evictions);
    CHECK(hits > 0 && evictions > 0);
    cache.clear();
    CHECK(d.alive.empty() && d.allocs == d.frees && cache.stats().evictions == evictions);
}

// A search larger than the budget: the first k chunks stay, the rest run uncached - the same this time and the next
static void check_partial_fit() {
    Device d;
    TemplCache cache;
    attach(cache, d);
    const size_t B = 1000;
    cache.set_budget(2 * B + 10);
    std::vector<Chunk> chunks;
    std::vector<TemplKey> keys;
    for (int i = 0; i < 5; ++i) {
        chunks.push_back(make_chunk(1, 1, 300 + i));
        chunks.back().in.dx = 2.0 + i;
        keys.push_back(key_of(chunks.back()));
    }
    for (int search = 0; search < 3; ++search) {
        cache.begin_search();
        for (int i = 0; i < 5; ++i) {
            TemplEntry* e = cache.find(keys[i]);
            if (!e) e = cache.insert(keys[i], B, 1);
            CHECK((e != nullptr) == (i < 2));
            check_invariants(cache, d);
        }
        const TemplCacheStats s = cache.stats();
        CHECK(s.hits == 2 * search && s.misses == 5 + 3 * search && s.entries == 2 && s.evictions == 0);
    }
    // another search (other keys) takes the room of the old one, least recently used first
    std::vector<Chunk> other;
    cache.begin_search();
    for (int i = 0; i < 2; ++i) {
        other.push_back(make_chunk(1, 1, 400 + i));
        other.back().in.dy = 7.0 + i;
        CHECK(cache.insert(key_of(other.back()), B, 1) != nullptr);
        check_invariants(cache, d);
    }
    CHECK(cache.stats().evictions == 2 && cache.find(keys[0]) == nullptr && cache.find(keys[1]) == nullptr);
    // an entry larger than the budget is never made; nor one the device has no memory for
    cache.begin_search();
    CHECK(cache.insert(keys[0], 2 * B + 11, 1) == nullptr);
    CHECK(d.largest <= cache.budget);
    d.cap = d.bytes;                                         // the device is full
    cache.begin_search();
    CHECK(cache.insert(keys[1], 10, 1) == nullptr);
    d.cap = (size_t)-1;
    check_invariants(cache, d);
    // allocation pressure: entries go one by one, the one in use last of all (and not at all while it is `keep`)
    const TemplEntry* keep = &cache.lru.front();
    while (cache.drop_lru(keep, true)) check_invariants(cache, d);
    CHECK(cache.lru.size() == 1 && &cache.lru.front() == keep);
    CHECK(cache.drop_lru(nullptr, true) && cache.lru.empty());
    // a smaller budget drops what no longer fits; 0 turns the cache off
    cache.set_budget(3 * B);
    cache.begin_search();
    for (int i = 0; i < 3; ++i) CHECK(cache.insert(keys[i], B, 1) != nullptr);
    cache.set_budget(B);
    CHECK(cache.lru.size() == 1 && cache.lru.front().key.equal(keys[2]));
    check_invariants(cache, d);
    cache.set_budget(0);
    CHECK(cache.lru.empty() && cache.insert(keys[0], 1, 1) == nullptr);
    // an entry whose planes were never completed is taken back
    cache.set_budget(3 * B);
    cache.begin_search();
    const long long ev = cache.stats().evictions;
    TemplEntry* e = cache.insert(keys[3], B, 1);
    CHECK(e != nullptr);
    cache.discard(e);
    CHECK(cache.find(keys[3]) == nullptr && cache.stats().evictions == ev);
    check_invariants(cache, d);
    cache.clear();
    CHECK(d.alive.empty() && d.allocs == d.frees && d.bad_frees == 0);
}

int main() {
    check_keys();
    for (int k = 1; k <= 4; ++k)
        for (unsigned seed = 1; seed <= 5; ++seed) check_lru(k, k + 1 + (int)seed % 3, 1000 * k + seed);
    check_partial_fit();
    std::printf("templ_cache_check: %lld checks, %lld failed\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
