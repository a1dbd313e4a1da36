// bmx/sv_algo.hpp -- which rows differ between two device-resident bit-sliced columns, header-only over bmx.h.
//
//   reference (src/bmsparsevec_algo.h)                                   here (two bound bmx::slice_scanner objects)
//   -------------------------------------------------------------------  ---------------------------------------------------
//   bm::sparse_vector_find_mismatch(bv, sv1, sv2, null_proc)   :656-792   bmx::sparse_vector_find_mismatch(bv, a, b, null_proc)
//   bm::sparse_vector_find_first_mismatch(sv1, sv2, midx,      :478-636   bmx::sparse_vector_find_first_mismatch(a, b, midx,
//                                         null_proc = use_null)                                                  null_proc = use_null)
//   (bv.count() of the first)                                             bmx::sparse_vector_count_mismatch(a, b, null_proc)
//
// One pass over both columns' planes (bmx_slice_mismatch / bmx_slice_first_mismatch, bmx_kernels17.h) where the reference runs a
// whole-vector XOR and OR per plane and up to three more passes for the NULL rule.  The two functions follow DIFFERENT rules in
// the reference (the first mismatch has no NULL masking and no size-difference term); both are kept as they are -- include/bmx.h
// spells them out, with the two differences: use_null without a not-NULL vector on either side is an error in the vector form
// (bmx::error with status BMX_ERR_BADARG), and the result's blocks are stored by content, not as bit-blocks.
// Host containers (two bm::sparse_vector<>) go through the overloads of bm_adapter.hpp.
#pragma once

#include <vector>

#include "scanner.hpp"

namespace bmx {

enum null_support { use_null = BMX_USE_NULL, no_null = BMX_NO_NULL };     // bm::null_support (src/bmconst.h:231)

namespace detail {
struct mismatch_args {
    std::vector<const bmx_vec*> ha, hb;
    const bmx_vec* na; const bmx_vec* nb;
    mismatch_args(const slice_scanner& a, const slice_scanner& b)
        : ha(a.slices().size() ? a.slices().size() : 1, nullptr), hb(b.slices().size() ? b.slices().size() : 1, nullptr),
          na(handle_or_null(a.not_null())), nb(handle_or_null(b.not_null()))
    {
        for (size_t i = 0; i < a.slices().size(); ++i) ha[i] = handle_or_null(a.slices()[i]);
        for (size_t i = 0; i < b.slices().size(); ++i) hb[i] = handle_or_null(b.slices()[i]);
    }
};
} // namespace detail

/// bv = the rows in which the two columns differ (:656)
inline void sparse_vector_find_mismatch(bvector& bv, const slice_scanner& a, const slice_scanner& b, null_support null_proc)
{
    detail::mismatch_args m(a, b);
    bmx_vec* r = nullptr;
    check(bmx_slice_mismatch(a.ctx().handle(), m.ha.data(), a.effective_slices(), a.size(), m.na,
                             m.hb.data(), b.effective_slices(), b.size(), m.nb, (int)null_proc, &r, nullptr));
    bv.adopt(r);
}

/// the number of rows sparse_vector_find_mismatch would set; nothing is materialised
inline size_type sparse_vector_count_mismatch(const slice_scanner& a, const slice_scanner& b, null_support null_proc)
{
    detail::mismatch_args m(a, b);
    uint64_t c = 0;
    check(bmx_slice_mismatch(a.ctx().handle(), m.ha.data(), a.effective_slices(), a.size(), m.na,
                             m.hb.data(), b.effective_slices(), b.size(), m.nb, (int)null_proc, nullptr, &c));
    return c;
}

/// midx = the first row of the reference's first-mismatch rule (:478); false (midx untouched) when there is none
inline bool sparse_vector_find_first_mismatch(const slice_scanner& a, const slice_scanner& b, size_type& midx, null_support null_proc = use_null)
{
    detail::mismatch_args m(a, b);
    int found = 0; uint64_t idx = 0;
    check(bmx_slice_first_mismatch(a.ctx().handle(), m.ha.data(), a.effective_slices(), a.size(), m.na,
                                   m.hb.data(), b.effective_slices(), b.size(), m.nb, (int)null_proc, &found, &idx));
    if (found) midx = idx;
    return found != 0;
}

} // namespace bmx
