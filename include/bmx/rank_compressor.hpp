// bmx/rank_compressor.hpp -- bm::rank_compressor<BV> (src/bmalgo.h:452-707) over the C-ABI: whole vectors between the row space
// and the rank space of an index vector, on the device.  Plain C++17; included by bmx/bvector.hpp.
//
//   bmx::rank_compressor rc;
//   rc.compress(target, idx, src);              // bit r of target <- the r-th one of idx is set in src; count(idx) bits
//   rc.decompress(target, idx, src);            // the inverse; idx's size
//   rc.compress_by_source(target, idx, rs, src) // the same as compress, with idx's rs_index (the reference's argument order)
// The batch forms are the loops of rsc_sparse_vector::load_from / load_to (src/bmsparsevec_compr.h:1496-1541): every plane
// against one index in one call; a null plane stays null.  Semantics and limits: include/bmx.h, bmx_rank_compress.
#pragma once
#include "bvector.hpp"

namespace bmx {

class rank_compressor {
public:
    typedef bvector bvector_type;
    typedef rs_index rs_index_type;

    /// src/bmalgo.h:497.  optimize: the target's blocks by the rule of bit_import_u32 instead of bit-blocks
    void compress(bvector& bv_target, const bvector& bv_idx, const bvector& bv_src, bool optimize = false) const
    {
        one(bmx_rank_compress, bv_target, bv_idx, nullptr, bv_src, optimize);
    }
    /// src/bmalgo.h:571
    void decompress(bvector& bv_target, const bvector& bv_idx, const bvector& bv_src, const rs_index* rs_idx = nullptr,
                    bool optimize = false) const
    {
        one(bmx_rank_decompress, bv_target, bv_idx, rs_idx, bv_src, optimize);
    }
    /// src/bmalgo.h:625
    void compress_by_source(bvector& bv_target, const bvector& bv_idx, const rs_index& bc_idx, const bvector& bv_src,
                            bool optimize = false) const
    {
        one(bmx_rank_compress, bv_target, bv_idx, &bc_idx, bv_src, optimize);
    }
    /// every srcs[i] (null: an absent plane, targets[i] is left without a handle) against one index
    void compress_many(std::vector<bvector>& targets, const bvector& bv_idx, const std::vector<const bvector*>& srcs,
                       const rs_index* rs_idx = nullptr, bool optimize = false) const
    {
        many(bmx_rank_compress_many, targets, bv_idx, srcs, rs_idx, optimize);
    }
    void decompress_many(std::vector<bvector>& targets, const bvector& bv_idx, const std::vector<const bvector*>& srcs,
                         const rs_index* rs_idx = nullptr, bool optimize = false) const
    {
        many(bmx_rank_decompress_many, targets, bv_idx, srcs, rs_idx, optimize);
    }

private:
    typedef int (*one_fn)(bmx_ctx*, const bmx_vec*, const bmx_rs*, const bmx_vec*, int, bmx_vec**);
    typedef int (*many_fn)(bmx_ctx*, const bmx_vec*, const bmx_rs*, const bmx_vec* const*, size_t, int, bmx_vec**);

    static void need(const bvector& v, const char* what)
    {
        if (v.empty_handle()) throw std::invalid_argument(std::string("bmx::rank_compressor: ") + what + " holds no vector");
    }
    static void one(one_fn fn, bvector& bv_target, const bvector& bv_idx, const rs_index* rs, const bvector& bv_src, bool optimize)
    {
        need(bv_idx, "bv_idx"); need(bv_src, "bv_src");
        bmx_vec* r = nullptr;
        check(fn(bv_idx.get_context().handle(), bv_idx.handle(), rs ? rs->handle() : nullptr, bv_src.handle(), optimize ? 1 : 0, &r));
        bv_target.adopt(r);                 // (the result is built first: the target may be one of the operands)
    }
    static void many(many_fn fn, std::vector<bvector>& targets, const bvector& bv_idx, const std::vector<const bvector*>& srcs,
                     const rs_index* rs, bool optimize)
    {
        need(bv_idx, "bv_idx");
        std::vector<const bmx_vec*> in(srcs.size(), nullptr);
        for (size_t i = 0; i < srcs.size(); ++i) in[i] = (srcs[i] && !srcs[i]->empty_handle()) ? srcs[i]->handle() : nullptr;
        std::vector<bmx_vec*> out(srcs.size(), nullptr);
        if (!srcs.empty())
            check(fn(bv_idx.get_context().handle(), bv_idx.handle(), rs ? rs->handle() : nullptr, in.data(), in.size(), optimize ? 1 : 0,
                     out.data()));
        std::vector<bvector> res;
        res.reserve(out.size());
        for (size_t i = 0; i < out.size(); ++i) { res.emplace_back(bv_idx.get_context()); res.back().adopt(out[i]); }
        targets = std::move(res);
    }
};

} // namespace bmx
