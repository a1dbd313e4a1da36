// GPU test of bmx::sparse_vector_find_mismatch / _count_mismatch / _find_first_mismatch (include/bmx/sv_algo.hpp) against word
// loops over vectors of the C oracle: the rules of src/bmsparsevec_algo.h:656-792 and :478-636 on the planes' words.
// Built and run by tests/test_cpp_sv_algo.py (-m gpu).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bmx/sv_algo.hpp"
extern "C" {
#include "../../oracle/bmx_oracle.h"
}

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static const uint64_t SEED = 0x5EED5;
typedef std::vector<uint32_t> words;

// a column on both sides: the oracle's words per plane (empty = the plane does not exist) and the device vectors
struct column {
    uint64_t size = 0;
    std::vector<words> planes;
    words nn; bool has_nn = false;
    std::vector<bmx::bvector> store;
    std::vector<const bmx::bvector*> slices;
    const bmx::bvector* dnn = nullptr;
};

static words oracle_words(uint32_t id, uint32_t dq, uint64_t nbits, uint64_t nw)
{
    words g(nw), w(nw);
    bmo_gen_words(SEED, id, 0, dq, nbits, 0, nw, g.data());
    bmo_vec* v = bmo_vec_import(g.data(), nw, 1);                          // through an oracle vector and back
    bmo_vec_to_words(v, w.data(), nw);
    bmo_vec_free(v);
    return w;
}

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

static uint32_t ones_below(uint64_t n, size_t word)                        // word `word` of ones[0, n)
{
    const uint64_t lo = (uint64_t)word * 32;
    return n >= lo + 32 ? ~0u : (n <= lo ? 0u : ((1u << (n - lo)) - 1u));
}

// vector form: false when the rule has no vector result (use_null, no not-NULL vector)
static bool expect_vector(const column& a, const column& b, bmx::null_support np, size_t nw, words& M)
{
    const uint64_t lo = a.size < b.size ? a.size : b.size, hi = a.size < b.size ? b.size : a.size;
    M.assign(nw, 0);
    for (size_t w = 0; w < nw; ++w) {
        uint32_t d = 0;
        for (size_t i = 0; i < a.planes.size() || i < b.planes.size(); ++i) {
            const uint32_t x = (i < a.planes.size() && !a.planes[i].empty()) ? a.planes[i][w] : 0u;
            const uint32_t y = (i < b.planes.size() && !b.planes[i].empty()) ? b.planes[i][w] : 0u;
            d |= x ^ y;
        }
        d |= ones_below(hi, w) & ~ones_below(lo, w);
        const uint32_t na = a.has_nn ? a.nn[w] : 0u, nb = b.has_nn ? b.nn[w] : 0u;
        if (np == bmx::no_null) { if (a.has_nn || b.has_nn) d &= na | nb; }
        else if (a.has_nn && b.has_nn) d |= na ^ nb;
        else if (a.has_nn) d |= ones_below(a.size, w) & ~na;
        else if (b.has_nn) d |= ones_below(b.size, w) & ~nb;
        else return false;
        M[w] = d & ones_below(hi, w);
    }
    return true;
}

static bool expect_first(const column& a, const column& b, bmx::null_support np, size_t nw, uint64_t& idx)
{
    for (size_t w = 0; w < nw; ++w) {
        uint32_t d = 0;
        for (size_t i = 0; i < a.planes.size() || i < b.planes.size(); ++i) {
            const uint32_t x = (i < a.planes.size() && !a.planes[i].empty()) ? a.planes[i][w] : 0u;
            const uint32_t y = (i < b.planes.size() && !b.planes[i].empty()) ? b.planes[i][w] : 0u;
            d |= x ^ y;
        }
        if (np == bmx::use_null) {
            if (a.has_nn && b.has_nn) d |= a.nn[w] ^ b.nn[w];
            else if (a.has_nn) d |= a.nn[w] ^ ones_below(b.size, w);       // the OTHER column's size (:515-526)
            else if (b.has_nn) d |= b.nn[w] ^ ones_below(a.size, w);
        }
        if (d) { idx = (uint64_t)w * 32 + (uint64_t)__builtin_ctz(d); return true; }
    }
    return false;
}

static void compare(bmx::context& ctx, column& a, column& b, size_t nw)
{
    bmx::slice_scanner sa(ctx), sb(ctx);
    bind(ctx, a, sa); bind(ctx, b, sb);
    REQUIRE(sa.slices().size() == a.planes.size() && sb.not_null() == b.dnn && &sa.ctx() == &ctx);
    const bmx::null_support procs[2] = {bmx::use_null, bmx::no_null};
    for (bmx::null_support np : procs) {
        words M;
        uint64_t eidx = 0, gidx = 12345;
        const bool ef = expect_first(a, b, np, nw, eidx);
        const bool gf = bmx::sparse_vector_find_first_mismatch(sa, sb, gidx, np);
        REQUIRE(gf == ef && (ef ? gidx == eidx : gidx == 12345));
        if (np == bmx::use_null) { uint64_t d = 0; REQUIRE(bmx::sparse_vector_find_first_mismatch(sa, sb, d) == ef && (!ef || d == eidx)); }
        if (!expect_vector(a, b, np, nw, M)) {
            bool threw = false;
            try { bmx::bvector t(ctx); bmx::sparse_vector_find_mismatch(t, sa, sb, np); } catch (const bmx::error& e) { threw = e.status() == BMX_ERR_BADARG; }
            REQUIRE(threw);
            continue;
        }
        uint64_t pop = 0;
        for (uint32_t x : M) pop += (uint64_t)__builtin_popcount(x);
        bmx::bvector bv(ctx);
        bmx::sparse_vector_find_mismatch(bv, sa, sb, np);
        REQUIRE(bv.size() == (a.size < b.size ? b.size : a.size));
        REQUIRE(bv.count() == pop);
        words got(nw);
        bv.export_words(got.data(), nw);
        REQUIRE(got == M);
        REQUIRE(bmx::sparse_vector_count_mismatch(sa, sb, np) == pop);
    }
}

int main()
{
    bmx::context ctx(0);
    const uint64_t nbits = 3 * 65536 + 1000;                               // 4 blocks
    const size_t nw = 4 * 2048;
    column a, b;
    a.size = nbits; b.size = nbits - 679;
    const uint32_t dq[4] = {19661u, 40u, 60000u, 655u};                    // bit-blocks, GAP blocks, dense, sparse
    for (unsigned i = 0; i < 4; ++i) a.planes.push_back(oracle_words(i, dq[i], a.size, nw));
    for (unsigned i = 0; i < 4; ++i) {                                     // b: a's planes below its size, two of them changed in a few rows
        words w = a.planes[i];
        if (i & 1) { const words x = oracle_words(20 + i, 13u, b.size, nw); for (size_t k = 0; k < nw; ++k) w[k] ^= x[k]; }
        for (size_t k = 0; k < nw; ++k) w[k] &= ones_below(b.size, k);
        b.planes.push_back(w);
    }
    b.planes.push_back(words());                                           // plane 4 does not exist, plane 5 only in b
    b.planes.push_back(oracle_words(30, 7u, b.size, nw));
    a.nn = oracle_words(40, 59000u, a.size, nw);
    b.nn = oracle_words(41, 59000u, b.size, nw);
    for (int na = 0; na < 2; ++na)
        for (int nb = 0; nb < 2; ++nb) {
            a.has_nn = na != 0; b.has_nn = nb != 0;
            compare(ctx, a, b, nw);
            compare(ctx, b, a, nw);
        }
    // equal columns: nothing differs, no first mismatch; the same scanner against itself
    a.has_nn = true;
    column c;                                                              // (distinct handles with the same content)
    c.size = a.size; c.planes = a.planes; c.nn = a.nn; c.has_nn = true;
    compare(ctx, a, c, nw);
    {
        bmx::slice_scanner s(ctx);
        bind(ctx, a, s);
        uint64_t idx = 7;
        REQUIRE(!bmx::sparse_vector_find_first_mismatch(s, s, idx) && idx == 7);
        REQUIRE(bmx::sparse_vector_count_mismatch(s, s, bmx::use_null) == 0);
    }
    std::printf("test_sv_algo ok\n");
    return 0;
}
