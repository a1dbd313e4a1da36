// bmx/sv_algo.hpp -- which rows differ between two device-resident bit-sliced columns, header-only over bmx.h.
//
//   reference (src/bmsparsevec_algo.h)                                   here (two bound bmx::slice_scanner objects)
//   -------------------------------------------------------------------  ---------------------------------------------------
//   bm::sparse_vector_find_mismatch(bv, sv1, sv2, null_proc)   :656-792   bmx::sparse_vector_find_mismatch(bv, a, b, null_proc)
//   bm::sparse_vector_find_first_mismatch(sv1, sv2, midx,      :478-636   bmx::sparse_vector_find_first_mismatch(a, b, midx,
//                                         null_proc = use_null)                                                  null_proc = use_null)
//   (bv.count() of the first)                                             bmx::sparse_vector_count_mismatch(a, b, null_proc)
//   bm::set2set_11_transform<SV>                              :1890-2205  bmx::set2set_11_transform (a bound slice_scanner is the SV)
//        remap(bv_in, sv, bv_out) / remap(bv_in, bv_out) / run / attach_sv / remap(id_from, sv, id_to); get_bv_zero is not offered
//
// One pass over both columns' planes (bmx_slice_mismatch / bmx_slice_first_mismatch, bmx_kernels17.h) where the reference runs a
// whole-vector XOR and OR per plane and up to three more passes for the NULL rule.  The two functions follow DIFFERENT rules in
// the reference (the first mismatch has no NULL masking and no size-difference term); both are kept as they are -- include/bmx.h
// spells them out, with the two differences: use_null without a not-NULL vector on either side is an error in the vector form
// (bmx::error with status BMX_ERR_BADARG), and the result's blocks are stored by content, not as bit-blocks.
// The image of a row set under a relation column (set2set_11_transform) is built on the device from the values the planes hold
// (bmx_slice_remap, bmx_kernels19.h): no list crosses to the host.
// Host containers (bm::sparse_vector<>) go through the overloads of bm_adapter.hpp.
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

/// bm::set2set_11_transform<SV> (src/bmsparsevec_algo.h:1890-2205): bv_out = { sv[i] : i in bv_in, sv[i] not NULL }, the image
/// of a row set under a relation column; M:1 relations are ordinary input.  The column is a bound (unsigned) slice_scanner.
/// The image has max(nbits_out, largest value + 1) bits (set_nbits_out, default 0) and is stored by content.
class set2set_11_transform {
public:
    set2set_11_transform() noexcept {}
    set2set_11_transform(const set2set_11_transform&) = delete;
    void operator=(const set2set_11_transform&) = delete;

    /// attach_sv(sv_brel, compute_stats) :2047 (nullptr detaches); compute_stats is accepted and ignored: no pass needs it
    void attach_sv(const slice_scanner* sv_brel, bool compute_stats = false) noexcept { (void)compute_stats; sv_ = sv_brel; }

    /// remap(bv_in, sv_brel, bv_out) :2096
    void remap(const bvector& bv_in, const slice_scanner& sv_brel, bvector& bv_out) { image(&bv_in, sv_brel, bv_out); }
    /// remap(bv_in, bv_out) :2114 with the attached column; without one (or with an empty one) bv_out is cleared (:2119-2122)
    void remap(const bvector& bv_in, bvector& bv_out)
    {
        if (!sv_) { bv_out.clear(); rows_ = 0; return; }
        image(&bv_in, *sv_, bv_out);
    }
    /// run(bv_in, sv_brel, bv_out) :1960
    void run(const bvector& bv_in, const slice_scanner& sv_brel, bvector& bv_out) { remap(bv_in, sv_brel, bv_out); }

    /// remap(id_from, sv_brel, id_to) :2076: one element; false (id_to untouched) for a NULL row, a row at or beyond size() and
    /// an empty column
    bool remap(size_type id_from, const slice_scanner& sv_brel, size_type& id_to)
    {
        refuse_signed(sv_brel);
        if (id_from >= sv_brel.size()) return false;
        bvector one(sv_brel.ctx());
        one.set(&id_from, 1, BM_SORTED);
        std::vector<uint64_t> v;
        sv_brel.values(&one, v);
        if (v.empty()) return false;
        id_to = v[0];
        return true;
    }

    void set_nbits_out(size_type nbits) noexcept { nbits_out_ = nbits; }
    /// the rows the last remap translated: count(bv_in & not_null & [0, size))
    size_type rows_translated() const noexcept { return rows_; }

private:
    static void refuse_signed(const slice_scanner& sv)
    {
        if (sv.is_signed()) throw error(BMX_ERR_BADARG, "set2set_11_transform over a signed column: positions cannot be negative");
    }
    void image(const bvector* bv_in, const slice_scanner& sv, bvector& bv_out)
    {
        refuse_signed(sv);
        bv_out.clear(); rows_ = 0;
        if (bv_in && bv_in->empty_handle()) {                          // (a vector without content selects nothing)
            bmx_vec* r = nullptr;
            check(bmx_vec_from_indices(sv.ctx().handle(), nullptr, 4, 0, BMX_UNSORTED, nbits_out_, 0, &r));
            bv_out.adopt(r);
            return;
        }
        std::vector<const bmx_vec*> h(sv.slices().size() ? sv.slices().size() : 1, nullptr);
        for (size_t i = 0; i < sv.slices().size(); ++i) h[i] = detail::handle_or_null(sv.slices()[i]);
        bmx_vec* r = nullptr; uint64_t n = 0;
        check(bmx_slice_remap(sv.ctx().handle(), h.data(), sv.effective_slices(), sv.size(), detail::handle_or_null(sv.not_null()),
                              bv_in ? bv_in->handle() : nullptr, nbits_out_, 1, &r, &n));
        bv_out.adopt(r);
        rows_ = n;
    }

    const slice_scanner* sv_ = nullptr;
    size_type nbits_out_ = 0, rows_ = 0;
};

} // namespace bmx
