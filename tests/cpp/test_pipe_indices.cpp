// GPU test of aggregator::combine_and_sub_indices(pipe, offsets, ids) (include/bmx/bvector.hpp) and slice_scanner::
// find_eq_indices(values, n, offsets, ids) (include/bmx/scanner.hpp) against the C oracle: per group the ones of
// bmo_agg_and_sub(and, sub), per value the rows that hold it.  Built and run by tests/test_cpp_pipe_indices.py (-m gpu).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "bmx/scanner.hpp"
extern "C" {
#include "../../oracle/bmx_oracle.h"
}

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static const uint64_t SEED = 0x1D5;

static std::vector<uint64_t> ones_of(const bmo_vec* v, uint64_t nbits, uint64_t from = 0, uint64_t to = ~0ull)
{
    std::vector<uint32_t> w(((nbits + 65535) / 65536) * 2048);
    bmo_vec_to_words(v, w.data(), w.size());
    std::vector<uint64_t> out;
    for (size_t i = 0; i < w.size(); ++i)
        for (uint32_t x = w[i]; x; x &= x - 1) {
            const uint64_t p = (uint64_t)i * 32 + (uint64_t)__builtin_ctz(x);
            if (p >= from && p <= to) out.push_back(p);
        }
    return out;
}

typedef bmx::aggregator<>::pipeline<bmx::agg_opt_disable_bvects_and_counts> pipe_t;
typedef bmx::aggregator<>::pipeline<bmx::agg_run_options<false, false, true> > masked_pipe_t;

int main()
{
    bmx::context ctx(0);
    const uint64_t nbits = 9 * 65536 + 321;
    const uint64_t nw = ((nbits + 63) / 64) * 2;
    // 12 operands: dense bit-blocks (92 %), mid (30 %), sparse GAP blocks (0.2 %)
    const uint32_t dq[12] = {60000u, 60000u, 60000u, 60000u, 60000u, 60000u, 19661u, 19661u, 19661u, 120u, 120u, 120u};
    std::vector<std::unique_ptr<bmx::bvector> > gv;
    std::vector<bmo_vec*> pv;
    for (unsigned i = 0; i < 12; ++i) {
        std::vector<uint32_t> w(nw);
        bmo_gen_words(SEED, i, 0, dq[i], nbits, 0, nw, w.data());
        pv.push_back(bmo_vec_import(w.data(), nw, 1));
        gv.emplace_back(new bmx::bvector(ctx));
        bmx::bit_import_u32(*gv.back(), w.data(), nw, true);
    }
    // arg-groups: AND lists of 1 .. 6 operands, SUB lists of 0 .. 3; one group without an AND list
    const std::vector<std::vector<unsigned> > ands = {{0}, {0, 1}, {0, 1, 2, 3, 4, 5}, {6, 0}, {}, {9}, {1, 6, 7}, {2, 3}};
    const std::vector<std::vector<unsigned> > subs = {{}, {6}, {9, 10}, {7, 8, 11}, {0}, {0}, {}, {3}};
    auto fill = [&](auto& pipe) {
        for (size_t g = 0; g < ands.size(); ++g) {
            auto* ag = pipe.add();
            for (unsigned i : ands[g]) ag->add(gv[i].get(), 0);
            for (unsigned i : subs[g]) ag->add(gv[i].get(), 1);
        }
        pipe.complete();
    };
    auto expect = [&](uint64_t from, uint64_t to, std::vector<uint64_t>& off, std::vector<uint64_t>& ids) {
        off.assign(1, 0); ids.clear();
        for (size_t g = 0; g < ands.size(); ++g) {
            if (!ands[g].empty()) {
                std::vector<const bmo_vec*> a, s;
                for (unsigned i : ands[g]) a.push_back(pv[i]);
                for (unsigned i : subs[g]) s.push_back(pv[i]);
                bmo_vec* r = bmo_agg_and_sub(a.data(), a.size(), s.data(), s.size());
                for (uint64_t p : ones_of(r, nbits, from, to)) ids.push_back(p);
                bmo_vec_free(r);
            }
            off.push_back(ids.size());
        }
    };
    bmx::aggregator<> agg(ctx);
    std::vector<bmx::size_type> off, ids, eoff, eids;
    {
        pipe_t pipe(ctx);
        fill(pipe);
        expect(0, ~0ull, eoff, eids);
        REQUIRE(eoff[5] == eoff[4] && eids.size() > 100000);
        agg.combine_and_sub_indices(pipe, off, ids);
        REQUIRE(off == eoff && ids == eids);
        agg.combine_and_sub_indices(pipe, off, ids);                     // into the buffer of the first call
        REQUIRE(off == eoff && ids == eids);
        agg.set_range_hint(70000, 5 * 65536 + 9);                         // no search masks in the options: the hint is ignored
        agg.combine_and_sub_indices(pipe, off, ids);
        REQUIRE(off == eoff && ids == eids);
    }
    {
        masked_pipe_t pipe(ctx);
        fill(pipe);
        // a hint across blocks: block granularity, columns 1 .. 5
        agg.set_range_hint(70000, 5 * 65536 + 9);
        expect(1 * 65536, 6 * 65536 - 1, eoff, eids);
        agg.combine_and_sub_indices(pipe, off, ids);
        REQUIRE(off == eoff && ids == eids && !ids.empty() && ids.front() >= 65536);
        // a hint inside one block: bit-masked as well
        agg.set_range_hint(2 * 65536 + 100, 2 * 65536 + 40000);
        expect(2 * 65536 + 100, 2 * 65536 + 40000, eoff, eids);
        agg.combine_and_sub_indices(pipe, off, ids);
        REQUIRE(off == eoff && ids == eids && !ids.empty());
        // one whole block
        agg.set_range_hint(3 * 65536, 4 * 65536 - 1);
        expect(3 * 65536, 4 * 65536 - 1, eoff, eids);
        agg.combine_and_sub_indices(pipe, off, ids);
        REQUIRE(off == eoff && ids == eids);
        agg.reset_range_hint();
        expect(0, ~0ull, eoff, eids);
        agg.combine_and_sub_indices(pipe, off, ids);
        REQUIRE(off == eoff && ids == eids);
    }
    // the scanner batch: 6 planes (plane 4 absent) over 3 blocks of rows, NULL rows stored as 0
    {
        const size_t rows = 3 * 65536 - 19;
        std::vector<uint64_t> col(rows);
        std::vector<bool> isnull(rows);
        uint64_t x = 88172645463325252ull;
        for (size_t r = 0; r < rows; ++r) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            isnull[r] = (x >> 40) % 10 == 0;
            col[r] = isnull[r] ? 0 : ((x & 63u) & ~16ull);
        }
        const size_t pw = ((rows + 63) / 64) * 2;
        std::vector<std::unique_ptr<bmx::bvector> > planes;
        std::vector<const bmx::bvector*> pp;
        for (unsigned b = 0; b < 6; ++b) {
            std::vector<uint32_t> w(pw, 0);
            for (size_t r = 0; r < rows; ++r) if ((col[r] >> b) & 1u) w[r >> 5] |= 1u << (r & 31u);
            if (b == 4) { pp.push_back(nullptr); continue; }
            planes.emplace_back(new bmx::bvector(ctx));
            bmx::bit_import_u32(*planes.back(), w.data(), pw, true);
            pp.push_back(planes.back().get());
        }
        std::vector<uint32_t> nw32(pw, 0);
        for (size_t r = 0; r < rows; ++r) if (!isnull[r]) nw32[r >> 5] |= 1u << (r & 31u);
        bmx::bvector nn(ctx);
        bmx::bit_import_u32(nn, nw32.data(), pw, true);
        bmx::slice_scanner sc(ctx);
        sc.bind(pp, rows, &nn);
        const uint64_t values[] = {5, 0, 47, 16, 5, 63, 1, 0, 21, 40};           // repeats, zeros, 16 / 21 / 63: a set bit without a plane
        const size_t nv = sizeof(values) / sizeof(values[0]);
        eoff.assign(1, 0); eids.clear();
        for (size_t q = 0; q < nv; ++q) {
            for (size_t r = 0; r < rows; ++r) if (!isnull[r] && col[r] == values[q]) eids.push_back(r);
            eoff.push_back(eids.size());
        }
        REQUIRE(eoff[4] == eoff[3] && eoff[2] > eoff[1] && eoff[1] > 0);
        sc.find_eq_indices(values, nv, off, ids);
        REQUIRE(off == eoff && ids == eids);
        sc.find_eq_indices(values + 2, 1, off, ids);                             // one value with its own group: no splice
        REQUIRE(off.size() == 2 && off[1] == eoff[3] - eoff[2] && ids == std::vector<uint64_t>(eids.begin() + (long)eoff[2], eids.begin() + (long)eoff[3]));
        sc.find_eq_indices(values, 0, off, ids);
        REQUIRE(off.size() == 1 && off[0] == 0 && ids.empty());
    }
    for (bmo_vec* p : pv) bmo_vec_free(p);
    std::printf("test_pipe_indices ok\n");
    return 0;
}
