// GPU test of bmx::str_scanner (include/bmx/str_scanner.hpp) against plain loops over the strings: every method, with and without a
// remap table, the batch entry and the pipeline, the empty string with and without a not-NULL vector
// (src/bmsparsevec_algo.h:1194-1235, 2546-2588, 3263-3436).  Built and run by tests/test_cpp_str_scanner.py (-m gpu).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bmx/str_scanner.hpp"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

typedef std::vector<uint32_t> words;
typedef std::vector<std::string> strings;

static uint64_t rnd(uint64_t& s) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }

struct column {
    strings rows;                                                          // what the caller sees
    std::vector<uint8_t> null;                                             // 1 = NULL (the row is empty then)
    std::vector<uint8_t> remap;                                            // octets x 256, or empty
    size_t octets = 0;
    std::vector<bmx::bvector> store;
    std::vector<const bmx::bvector*> planes;
    const bmx::bvector* nn = nullptr;
};

// the column onto the device: plane octet * 8 + bit of the (remapped) characters, absent where no row sets it
static void bind(bmx::context& ctx, column& c, bmx::str_scanner& sc, bool with_nn, size_t extra_rows = 0)
{
    const size_t n = c.rows.size(), np = c.octets * 8, nw = ((n + extra_rows + 65535) / 65536) * 2048;
    std::vector<words> pw(np);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < c.rows[i].size(); ++j) {
            unsigned ch = (uint8_t)c.rows[i][j];
            if (!c.remap.empty()) ch = c.remap[j * 256 + ch];
            for (unsigned b = 0; b < 8; ++b) if ((ch >> b) & 1u) { words& w = pw[j * 8 + b]; if (w.empty()) w.assign(nw, 0); w[i >> 5] |= 1u << (i & 31); }
        }
    if (extra_rows) {                                                      // rows past size spell rows[0]: they must never count
        for (size_t i = n; i < n + extra_rows; ++i)
            for (size_t p = 0; p < np; ++p) if (!pw[p].empty() && ((pw[p][0] >> 0) & 1u)) pw[p][i >> 5] |= 1u << (i & 31);
    }
    c.store.clear(); c.store.reserve(np + 1);
    c.planes.assign(np, nullptr);
    for (size_t p = 0; p < np; ++p) {
        if (pw[p].empty()) continue;
        c.store.emplace_back(ctx);
        bmx::bit_import_u32(c.store.back(), pw[p].data(), pw[p].size(), true);
        c.planes[p] = &c.store.back();
    }
    c.nn = nullptr;
    if (with_nn) {
        words w(nw, 0);
        for (size_t i = 0; i < n; ++i) if (!c.null[i]) w[i >> 5] |= 1u << (i & 31);
        c.store.emplace_back(ctx);
        bmx::bit_import_u32(c.store.back(), w.data(), w.size(), true);
        c.nn = &c.store.back();
    }
    sc.bind(c.planes, n, c.nn);
    sc.set_remap(c.remap.empty() ? nullptr : c.remap.data(), c.octets);
}

static std::vector<uint64_t> loop_rows(const column& c, const std::string& s, bool prefix, bool with_nn)
{
    std::vector<uint64_t> out;
    for (size_t i = 0; i < c.rows.size(); ++i) {
        const bool hit = prefix ? c.rows[i].compare(0, s.size(), s) == 0 : c.rows[i] == s;
        if (hit && (prefix || !s.empty() || !with_nn || !c.null[i])) out.push_back(i);
    }
    return out;
}

static void check_all(bmx::context& ctx, column& c, const strings& queries, bool with_nn)
{
    bmx::str_scanner sc(ctx);
    bind(ctx, c, sc, with_nn, 100);
    const size_t n = queries.size();
    std::vector<std::vector<uint64_t>> exp(n);
    for (size_t q = 0; q < n; ++q) exp[q] = loop_rows(c, queries[q], false, with_nn);
    // single searches
    for (size_t q = 0; q < n; ++q) {
        bmx::bvector bv(ctx);
        const bool f = sc.find_eq_str(queries[q].c_str(), bv);
        std::vector<bmx::size_type> got;
        if (f) bv.to_indices(got);
        REQUIRE(f == !exp[q].empty() && got == exp[q]);
        bmx::size_type pos = 0;
        const bool f1 = sc.find_eq_str(queries[q].c_str(), pos);
        REQUIRE(f1 == !exp[q].empty() && (!f1 || pos == exp[q][0]));
        bmx::bvector bp(ctx);
        const bool fp = sc.find_eq_str_prefix(queries[q].c_str(), bp);
        std::vector<uint64_t> ep = loop_rows(c, queries[q], true, with_nn);
        bool representable = true;                                         // a prefix the tables cannot spell is found nowhere
        if (!c.remap.empty()) for (size_t j = 0; j < queries[q].size(); ++j) if (j >= c.octets || !c.remap[j * 256 + (uint8_t)queries[q][j]]) representable = false;
        got.clear();
        if (fp) bp.to_indices(got);
        if (representable && queries[q].size() <= c.octets) REQUIRE(got == ep); else REQUIRE(got.empty());
    }
    // batches: the entry (automatic from BATCH_MIN strings upward) and the pipeline
    REQUIRE(n >= bmx::str_scanner::BATCH_MIN);
    for (int pipe = 0; pipe < 2; ++pipe) {
        std::vector<uint64_t> counts;
        sc.find_eq_str_counts(queries, counts, pipe != 0);
        std::vector<bmx::size_type> pos; std::vector<uint8_t> found;
        sc.find_eq_str_first(queries, pos, found, pipe != 0);
        REQUIRE(counts.size() == n && pos.size() == n && found.size() == n);
        for (size_t q = 0; q < n; ++q) {
            REQUIRE(counts[q] == exp[q].size());
            REQUIRE((found[q] != 0) == !exp[q].empty() && pos[q] == (exp[q].empty() ? 0 : exp[q][0]));
        }
    }
    strings few(queries.begin(), queries.begin() + 3);                     // a short batch takes the pipeline by itself
    std::vector<uint64_t> cf;
    sc.find_eq_str_counts(few, cf);
    for (size_t q = 0; q < 3; ++q) REQUIRE(cf[q] == exp[q].size());
    std::vector<bmx::size_type> off, ids;
    sc.find_eq_str_indices(queries, off, ids);
    REQUIRE(off.size() == n + 1 && off[0] == 0);
    for (size_t q = 0; q < n; ++q) {
        REQUIRE(off[q + 1] - off[q] == exp[q].size());
        REQUIRE(std::equal(exp[q].begin(), exp[q].end(), ids.begin() + (ptrdiff_t)off[q]));
    }
    strings none;
    std::vector<uint64_t> c0;
    sc.find_eq_str_counts(none, c0);
    REQUIRE(c0.empty());
}

int main()
{
    bmx::context ctx(0);
    static const char* const pool[] = {"ga", "tag", "gat", "a", "tt", "gattaca", "tagg", "c", "ac", "ca", "ab", "abc"};
    const size_t npool = sizeof(pool) / sizeof(pool[0]);
    column c;
    c.octets = 8;
    uint64_t s = 0x57125EA7C4;
    const size_t n = 65536 + 4321;
    c.rows.resize(n); c.null.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint64_t r = rnd(s);
        if (r % 97 == 0) { c.rows[i] = ""; c.null[i] = (r >> 20) & 1; }
        else c.rows[i] = pool[(r >> 8) % (npool - 2)];                     // "ab" / "abc": rows 10 and 11 only
    }
    c.rows[10] = "ab"; c.rows[11] = "abc"; c.null[10] = c.null[11] = 0;
    strings queries;
    for (size_t i = 0; i < npool; ++i) queries.push_back(pool[i]);
    const char* const more[] = {"", "g", "gatt", "gattacaa", "gattacaaa", "x", "t", "tagga", "ga", ""};
    for (size_t i = 0; i < sizeof(more) / sizeof(more[0]); ++i) queries.push_back(more[i]);
    while (queries.size() < 3 * bmx::str_scanner::BATCH_MIN / 2) {        // enough for the batch entry: pool strings with a letter changed, appended or cut
        const uint64_t r = rnd(s);
        std::string q = pool[r % npool];
        if ((r >> 8) & 1) q[(r >> 12) % q.size()] = "acgt"[(r >> 16) & 3];
        if ((r >> 9) & 1) q += "acgt"[(r >> 18) & 3];
        if (((r >> 10) & 3) == 0) q.erase(q.size() - 1);
        queries.push_back(q);
    }
    check_all(ctx, c, queries, true);
    check_all(ctx, c, queries, false);
    // the same column as codes: one table per octet position, codes by first appearance
    c.remap.assign(c.octets * 256, 0);
    std::vector<unsigned> next(c.octets, 1);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < c.rows[i].size(); ++j) { uint8_t& e = c.remap[j * 256 + (uint8_t)c.rows[i][j]]; if (!e) e = (uint8_t)next[j]++; }
    check_all(ctx, c, queries, true);
    check_all(ctx, c, queries, false);
    std::printf("test_str_scanner ok\n");
    return 0;
}
