// GPU test of bmx::set2set_11_transform and bmx::slice_scanner::values (include/bmx/sv_algo.hpp, include/bmx/scanner.hpp) against
// plain loops over the words of vectors of the C oracle: the rows bv_in & not_null & [0, size), their values from the planes'
// bits, and the set of those values (src/bmsparsevec_algo.h:2096-2205).  Built and run by tests/test_cpp_set2set.py (-m gpu).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bmx/sv_algo.hpp"
extern "C" {
#include "../../oracle/bmx_oracle.h"
}

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static const uint64_t SEED = 0x5E25E7;
typedef std::vector<uint32_t> words;

static words oracle_words(uint32_t id, uint32_t dq, uint64_t nbits, uint64_t nw)
{
    words g(nw), w(nw);
    bmo_gen_words(SEED, id, 0, dq, nbits, 0, nw, g.data());
    bmo_vec* v = bmo_vec_import(g.data(), nw, 1);                          // through an oracle vector and back
    bmo_vec_to_words(v, w.data(), nw);
    bmo_vec_free(v);
    return w;
}

static bool bit(const words& w, uint64_t i) { return (i >> 5) < w.size() && ((w[i >> 5] >> (i & 31)) & 1u); }

struct column {
    uint64_t size = 0;
    std::vector<words> planes;                                             // empty = the plane does not exist
    words nn; bool has_nn = false;
    std::vector<bmx::bvector> store;
    std::vector<const bmx::bvector*> slices;
    const bmx::bvector* dnn = nullptr;
};

static void bind(bmx::context& ctx, column& c, bmx::slice_scanner& sc)
{
    c.store.clear(); c.store.reserve(c.planes.size() + 1);
    c.slices.assign(c.planes.size(), nullptr);
    for (size_t i = 0; i < c.planes.size(); ++i) {
        if (c.planes[i].empty()) continue;
        c.store.emplace_back(ctx);
        bmx::bit_import_u32(c.store.back(), c.planes[i].data(), c.planes[i].size(), true);
        c.slices[i] = &c.store.back();
    }
    c.dnn = nullptr;
    if (c.has_nn) {
        c.store.emplace_back(ctx);
        bmx::bit_import_u32(c.store.back(), c.nn.data(), c.nn.size(), true);
        c.dnn = &c.store.back();
    }
    sc.bind(c.slices, c.size, c.dnn);
}

// the plain loop: rows, values by row, and the sorted distinct values
static void expect(const column& c, const words* sel, std::vector<uint64_t>& rows, std::vector<uint64_t>& vals, std::vector<uint64_t>& image)
{
    rows.clear(); vals.clear();
    for (uint64_t i = 0; i < c.size; ++i) {
        if (sel && !bit(*sel, i)) continue;
        if (c.has_nn && !bit(c.nn, i)) continue;
        uint64_t v = 0;
        for (size_t p = 0; p < c.planes.size(); ++p) if (!c.planes[p].empty() && bit(c.planes[p], i)) v |= 1ull << p;
        rows.push_back(i); vals.push_back(v);
    }
    image = vals;
    std::sort(image.begin(), image.end());
    image.erase(std::unique(image.begin(), image.end()), image.end());
}

static void run_case(bmx::context& ctx, column& c, const words* sel, const char* name)
{
    bmx::slice_scanner sc(ctx);
    bind(ctx, c, sc);
    bmx::bvector d_sel(ctx);
    if (sel) bmx::bit_import_u32(d_sel, sel->data(), sel->size(), true);
    std::vector<uint64_t> rows, vals, image;
    expect(c, sel, rows, vals, image);
    std::vector<uint64_t> gv; std::vector<bmx::size_type> gr;
    sc.values(sel ? &d_sel : nullptr, gv, &gr);
    REQUIRE(gv == vals); REQUIRE(gr == rows);
    sc.values(sel ? &d_sel : nullptr, gv);
    REQUIRE(gv == vals);
    if (!sel) { std::printf("  %s: %zu rows (values only)\n", name, rows.size()); return; }
    bmx::set2set_11_transform t;
    bmx::bvector out(ctx), out2(ctx), out3(ctx);
    t.remap(d_sel, sc, out);
    std::vector<bmx::size_type> ids;
    out.to_indices(ids);
    REQUIRE(ids == image); REQUIRE(t.rows_translated() == rows.size());
    REQUIRE(out.size() == (image.empty() ? 0 : image.back() + 1));
    t.run(d_sel, sc, out2);
    out2.to_indices(ids); REQUIRE(ids == image);
    t.remap(d_sel, out3);                                                   // nothing attached: cleared
    REQUIRE(out3.empty_handle());
    t.attach_sv(&sc, true);
    t.set_nbits_out(70000);
    t.remap(d_sel, out3);
    out3.to_indices(ids); REQUIRE(ids == image);
    REQUIRE(out3.size() == std::max<uint64_t>(70000, image.empty() ? 0 : image.back() + 1));
    t.attach_sv(nullptr);
    // single elements: a selected row, a NULL row, a row beyond the column
    for (uint64_t i = 0; i < c.size; i += c.size / 7 + 1) {
        bmx::size_type to = 12345;
        uint64_t v = 0;
        for (size_t p = 0; p < c.planes.size(); ++p) if (!c.planes[p].empty() && bit(c.planes[p], i)) v |= 1ull << p;
        const bool valid = !c.has_nn || bit(c.nn, i);
        REQUIRE(t.remap(i, sc, to) == valid);
        REQUIRE(to == (valid ? v : 12345));
    }
    bmx::size_type to = 777;
    REQUIRE(!t.remap(c.size, sc, to) && to == 777);
    std::printf("  %s: %zu rows -> %zu values\n", name, rows.size(), image.size());
}

int main()
{
    bmx::context ctx(0);
    const uint64_t B = 65536;
    // 1. five planes (one absent, one two blocks shorter), a not-NULL vector, a dense selector longer than the column
    {
        column c; c.size = 4 * B + 1000;
        const uint64_t nw = 5 * 2048;
        c.planes.resize(5);
        c.planes[0] = oracle_words(1, 20000, c.size, nw);
        c.planes[1] = oracle_words(2, 300, c.size, nw);
        c.planes[3] = oracle_words(3, 40000, 2 * B + 5, 3 * 2048);
        c.planes[4] = oracle_words(4, 6554, c.size, nw);
        c.nn = oracle_words(5, 50000, c.size, nw); c.has_nn = true;
        words sel = oracle_words(6, 30000, 6 * B, 6 * 2048);
        run_case(ctx, c, &sel, "five planes, dense selector past the end");
        words sparse = oracle_words(7, 200, c.size, nw);
        run_case(ctx, c, &sparse, "five planes, sparse selector");
        run_case(ctx, c, nullptr, "five planes, every row");
        c.has_nn = false;
        run_case(ctx, c, &sel, "five planes, no not-NULL vector");
    }
    // 2. 40 planes of one block: width 8 inside, values below 2^36 (planes 36.. are absent)
    {
        column c; c.size = B - 100;
        c.planes.resize(40);
        for (uint32_t i = 0; i < 36; ++i) c.planes[i] = oracle_words(100 + i, 6554 * (1 + i % 9), c.size, 2048);
        words sel = oracle_words(150, 3000, c.size, 2048);
        run_case(ctx, c, &sel, "40 planes");
    }
    // 3. no planes: the image is {0} iff a row is selected; an all-clear selector
    {
        column c; c.size = B + 9;
        words sel = oracle_words(160, 100, c.size, 2 * 2048), none(2 * 2048, 0u);
        run_case(ctx, c, &sel, "no planes");
        run_case(ctx, c, &none, "nothing selected");
    }
    // 4. a signed scanner: values() converts the s2u patterns, the transform refuses the column
    {
        column c; c.size = 64;
        c.planes.resize(3);
        for (uint32_t p = 0; p < 3; ++p) { c.planes[p].assign(2048, 0u); for (uint64_t i = 0; i < 64; ++i) if (((i % 8) >> p) & 1) c.planes[p][i >> 5] |= 1u << (i & 31); }
        bmx::slice_scanner sc(ctx);
        bind(ctx, c, sc);
        sc.set_signed(true);
        std::vector<uint64_t> gv;
        sc.values(nullptr, gv);
        REQUIRE(gv.size() == 64);
        for (uint64_t i = 0; i < 64; ++i) { const uint64_t u = i % 8; const int64_t want = (u & 1) ? -(int64_t)(u >> 1) - 1 : (int64_t)(u >> 1); REQUIRE((int64_t)gv[i] == want); }
        bmx::set2set_11_transform t;
        bmx::bvector in(ctx), out(ctx);
        bmx::size_type id = 3; in.set(&id, 1);
        int status = 0;
        try { t.remap(in, sc, out); } catch (const bmx::error& e) { status = e.status(); }
        REQUIRE(status == BMX_ERR_BADARG);
        status = 0;
        try { bmx::size_type to; t.remap(3, sc, to); } catch (const bmx::error& e) { status = e.status(); }
        REQUIRE(status == BMX_ERR_BADARG);
    }
    std::printf("test_set2set ok\n");
    return 0;
}
