// GPU test of bmx::rank_compressor (include/bmx/rank_compressor.hpp) against the C oracle: the reference's per-bit rule
// (src/bmalgo.h:673-674, :593-612) through the oracle's rank / select and set_bit, then optimize().
// Built and run by tests/test_cpp_rankc.py (-m gpu).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bmx/rank_compressor.hpp"
extern "C" {
#include "../../oracle/bmx_oracle.h"
}

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static const uint64_t SEED = 0xC0FFEE;

static std::vector<uint64_t> ones_of(const bmo_vec* v, uint64_t nbits)
{
    std::vector<uint32_t> w(((nbits + 65535) / 65536) * 2048);
    bmo_vec_to_words(v, w.data(), w.size());
    std::vector<uint64_t> out;
    for (size_t i = 0; i < w.size(); ++i)
        for (uint32_t x = w[i]; x; x &= x - 1) out.push_back((uint64_t)i * 32 + (uint64_t)__builtin_ctz(x));
    return out;
}

// the device vector against the oracle vector: size, count, words; with optimize also the block kinds
static void same(const bmx::bvector& g, bmo_vec* e, uint64_t nbits, bool optimize)
{
    REQUIRE(g.size() == nbits);
    REQUIRE(g.count() == bmo_vec_count(e));
    const uint64_t nw = ((nbits + 65535) / 65536) * 2048;
    std::vector<uint32_t> w1(nw), w2(nw);
    if (nw) { g.export_words(w1.data(), nw); bmo_vec_to_words(e, w2.data(), nw); }
    REQUIRE(w1 == w2);
    if (optimize) {
        bmo_vec_optimize(e);
        bmx::bvector::statistics st; g.calc_stat(&st);
        uint32_t c[4]; uint64_t gw; bmo_vec_stat(e, c, &gw);
        REQUIRE(st.bit_blocks == c[BMO_BIT] && st.gap_blocks == c[BMO_GAP] && st.full_blocks == c[BMO_FULL]);
    }
}

int main()
{
    bmx::context ctx(0);
    const uint64_t nbits = 9 * 65536 + 321;
    const uint64_t nw = ((nbits + 63) / 64) * 2;
    const uint64_t vbits = nw * 32;                                        // bit_import_u32 sizes a vector by its words
    const uint32_t idx_dq[3] = {19661u, 655u, 60000u};                     // 30 %, 1 %, 92 %
    const uint32_t src_dq[4] = {6554u, 120u, 32768u, 65536u};
    bmx::rank_compressor rc;
    for (unsigned i = 0; i < 3; ++i) {
        std::vector<uint32_t> iw(nw);
        bmo_gen_words(SEED, i, 0, idx_dq[i], nbits, 0, nw, iw.data());
        bmo_vec* pidx = bmo_vec_import(iw.data(), nw, 1);
        bmo_rs* prs = bmo_rs_build(pidx);
        const uint64_t cnt = bmo_rs_count(prs);
        bmx::bvector idx(ctx);
        bmx::bit_import_u32(idx, iw.data(), nw, true);
        bmx::rs_index rs;
        idx.build_rs_index(&rs);
        REQUIRE(rs.count() == cnt);
        std::vector<bmx::bvector> srcs;
        std::vector<bmo_vec*> psrcs;
        for (unsigned j = 0; j < 4; ++j) {
            std::vector<uint32_t> sw(nw);
            bmo_gen_words(SEED, 10 + j, 0, src_dq[j], nbits, 0, nw, sw.data());
            psrcs.push_back(bmo_vec_import(sw.data(), nw, 1));
            srcs.emplace_back(ctx);
            bmx::bit_import_u32(srcs.back(), sw.data(), nw, true);
        }
        for (int optimize = 0; optimize < 2; ++optimize) {
            std::vector<const bmx::bvector*> in;
            for (unsigned j = 0; j < 4; ++j) {
                // compress: bit count_to(p) - 1 for every one p of src & idx
                bmo_vec* both = bmo_op2(0, psrcs[j], pidx, 0);
                bmo_vec* e = bmo_vec_new(cnt);
                for (uint64_t p : ones_of(both, nbits)) bmo_vec_set_bit(e, bmo_rank(pidx, prs, p) - 1);
                bmx::bvector t(ctx), t2(ctx);
                rc.compress(t, idx, srcs[j], optimize != 0);
                rc.compress_by_source(t2, idx, rs, srcs[j], optimize != 0);
                REQUIRE(t.equal(t2));
                same(t, e, cnt, optimize != 0);
                // decompress of the result: src & idx
                bmx::bvector back(ctx);
                rc.decompress(back, idx, t, &rs, optimize != 0);
                same(back, both, vbits, optimize != 0);
                // decompress of src itself: bit select(s + 1) for every one s of src below count(idx)
                bmo_vec* d = bmo_vec_new(vbits);
                for (uint64_t s : ones_of(psrcs[j], nbits)) {
                    if (s >= cnt) break;
                    uint64_t pos = 0;
                    REQUIRE(bmo_select(pidx, prs, s + 1, &pos));
                    bmo_vec_set_bit(d, pos);
                }
                bmx::bvector dec(ctx);
                rc.decompress(dec, idx, srcs[j], nullptr, optimize != 0);
                same(dec, d, vbits, optimize != 0);
                bmo_vec_free(both); bmo_vec_free(e); bmo_vec_free(d);
                in.push_back(&srcs[j]);
                if (j == 1) in.push_back(nullptr);
            }
            // the batch forms: every target equals the single call; an absent plane stays without a handle
            std::vector<bmx::bvector> outs;
            rc.compress_many(outs, idx, in, &rs, optimize != 0);
            REQUIRE(outs.size() == in.size());
            for (size_t k = 0; k < in.size(); ++k) {
                if (!in[k]) { REQUIRE(outs[k].empty_handle()); continue; }
                bmx::bvector one(ctx);
                rc.compress(one, idx, *in[k], optimize != 0);
                REQUIRE(outs[k].equal(one));
            }
            rc.decompress_many(outs, idx, in, nullptr, optimize != 0);
            for (size_t k = 0; k < in.size(); ++k) {
                if (!in[k]) { REQUIRE(outs[k].empty_handle()); continue; }
                bmx::bvector one(ctx);
                rc.decompress(one, idx, *in[k], &rs, optimize != 0);
                REQUIRE(outs[k].equal(one));
            }
        }
        // the target may be an operand; an empty handle is refused
        bmx::bvector t(ctx);
        rc.compress(t, idx, srcs[0]);
        const uint64_t c0 = t.count();
        rc.decompress(t, idx, t);
        REQUIRE(t.size() == vbits && t.count() == c0);
        bool threw = false;
        try { bmx::bvector none(ctx), o(ctx); rc.compress(o, idx, none); } catch (const std::invalid_argument&) { threw = true; }
        REQUIRE(threw);
        for (bmo_vec* p : psrcs) bmo_vec_free(p);
        bmo_rs_free(prs); bmo_vec_free(pidx);
    }
    std::printf("test_rank_compressor ok\n");
    return 0;
}
