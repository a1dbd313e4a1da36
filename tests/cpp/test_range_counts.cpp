// GPU test of bmx::slice_scanner::find_range_counts / histogram (include/bmx/scanner.hpp -> bmx_slice_range_counts) against a
// row loop over the values the planes spell, and against the loop of count(BMX_CMP_RANGE, ..) calls they replace
// (sparse_vector_scanner::find_range + count(), src/bmsparsevec_algo.h:2862).  Planes come from the C oracle's generator.
// Built and run by tests/test_cpp_range_counts.py (-m gpu).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bmx/scanner.hpp"
extern "C" {
#include "../../oracle/bmx_oracle.h"
}

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static const uint64_t SEED = 0x5EED7;
typedef std::vector<uint32_t> words;

static words oracle_words(uint32_t id, uint32_t dq, uint64_t nbits, uint64_t nw)
{
    words g(nw), w(nw);
    bmo_gen_words(SEED, id, 0, dq, nbits, 0, nw, g.data());
    bmo_vec* v = bmo_vec_import(g.data(), nw, 1);
    bmo_vec_to_words(v, w.data(), nw);
    bmo_vec_free(v);
    return w;
}

static uint64_t model(const std::vector<uint64_t>& val, const std::vector<bool>& valid, uint64_t lo, uint64_t hi)
{
    if (hi < lo) { const uint64_t t = lo; lo = hi; hi = t; }
    uint64_t c = 0;
    for (size_t i = 0; i < val.size(); ++i) c += valid[i] && lo <= val[i] && val[i] <= hi;
    return c;
}

static void run(bmx::context& ctx, bool with_nn)
{
    const uint64_t size = 3 * 65536 + 1000;                                // 4 blocks
    const size_t nw = 4 * 2048;
    const uint32_t dq[6] = {32768u, 19661u, 40u, 60000u, 0u, 655u};        // bit-blocks, GAP blocks, dense, absent (plane 4), sparse
    std::vector<words> planes(6);
    words nn = oracle_words(40, 59000u, size, nw);
    for (unsigned i = 0; i < 6; ++i) {
        if (!dq[i]) continue;
        planes[i] = oracle_words(i, dq[i], size, nw);
        if (with_nn) for (size_t k = 0; k < nw; ++k) planes[i][k] &= nn[k];   // a NULL row holds 0
    }
    std::vector<uint64_t> val(size, 0); std::vector<bool> valid(size, true);
    for (uint64_t r = 0; r < size; ++r) {
        for (unsigned i = 0; i < 6; ++i) if (!planes[i].empty() && ((planes[i][r >> 5] >> (r & 31)) & 1u)) val[r] |= 1ull << i;
        if (with_nn) valid[r] = ((nn[r >> 5] >> (r & 31)) & 1u) != 0;
    }
    std::vector<bmx::bvector> store; store.reserve(7);
    std::vector<const bmx::bvector*> slices(6, nullptr);
    for (unsigned i = 0; i < 6; ++i) {
        if (planes[i].empty()) continue;
        store.emplace_back(ctx);
        bmx::bit_import_u32(store.back(), planes[i].data(), planes[i].size(), true);
        slices[i] = &store.back();
    }
    const bmx::bvector* dnn = nullptr;
    if (with_nn) { store.emplace_back(ctx); bmx::bit_import_u32(store.back(), nn.data(), nn.size(), true); dnn = &store.back(); }
    bmx::slice_scanner sc(ctx);
    sc.bind(slices, size, dnn);

    // 40 ranges (more thresholds than one launch holds): overlapping, reversed, duplicated, with bounds above every plane
    std::vector<uint64_t> lo, hi;
    for (uint64_t k = 0; k < 18; ++k) { lo.push_back(k * 3); hi.push_back(k * 3 + (k % 5)); }
    for (uint64_t k = 0; k < 18; ++k) { lo.push_back(63 - k); hi.push_back(k); }
    lo.push_back(0); hi.push_back(~0ull);
    lo.push_back(0); hi.push_back(0);
    lo.push_back(64); hi.push_back(1ull << 40);
    lo.push_back(7); hi.push_back(7);
    std::vector<uint64_t> got(lo.size(), 12345);
    sc.find_range_counts(lo.data(), hi.data(), lo.size(), got.data());
    bool some = false, none = false;
    for (size_t q = 0; q < lo.size(); ++q) {
        const uint64_t e = model(val, valid, lo[q], hi[q]);
        REQUIRE(got[q] == e);
        REQUIRE(sc.count(BMX_CMP_RANGE, lo[q], hi[q]) == e);               // the loop this call replaces
        some |= e != 0; none |= e == 0;
    }
    REQUIRE(some && none);
    uint64_t poison = 777;
    sc.find_range_counts(lo.data(), hi.data(), 0, &poison);                // n = 0: nothing is written
    REQUIRE(poison == 777);

    // histogram: bins [e[k], e[k + 1]), a repeated edge gives an empty bin, the bins sum to the rows in [e[0], e[last])
    const uint64_t edges[] = {0, 1, 1, 5, 16, 17, 40, 64, 64, 1000};
    const size_t ne = sizeof(edges) / sizeof(edges[0]);
    std::vector<uint64_t> bins(ne - 1, 12345);
    sc.histogram(edges, ne, bins.data());
    uint64_t sum = 0;
    for (size_t k = 0; k + 1 < ne; ++k) {
        REQUIRE(bins[k] == (edges[k] == edges[k + 1] ? 0 : model(val, valid, edges[k], edges[k + 1] - 1)));
        sum += bins[k];
    }
    REQUIRE(sum == model(val, valid, edges[0], edges[ne - 1] - 1));
    bool threw = false;
    const uint64_t bad[] = {5, 3};
    try { sc.histogram(bad, 2, bins.data()); } catch (const bmx::error& e) { threw = e.status() == BMX_ERR_BADARG; }
    REQUIRE(threw);
}

int main()
{
    bmx::context ctx(0);
    run(ctx, false);
    run(ctx, true);
    std::printf("test_range_counts ok\n");
    return 0;
}
