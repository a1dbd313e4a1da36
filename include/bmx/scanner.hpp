// bmx/scanner.hpp -- bit-sliced equality search over device-resident slices: the aggregator call
// pattern of bm::sparse_vector_scanner<SV>, header-only over bmx.h.
//
//   reference                                                     here
//   ------------------------------------------------------------  ----------------------------------
//   sparse_vector_scanner::find_eq(sv, value, bv_out)             slice_scanner::find_eq(value, bv_out)
//        src/bmsparsevec_algo.h:1083,4356 -> find_eq_with_nulls :2387-2412
//   sparse_vector_scanner::find_eq(sv, value, pos) :1111,4434     slice_scanner::find_first_eq(value, idx)
//        -> find_first_eq :2417
//   prepare_and_sub_aggregator(sv, value) :2593-2640              slice_scanner::add_groups()
//        AND group = slices of the set bits of the value (high bit first),
//        SUB group = every other existing slice below effective_slices(); a set bit
//        without a slice => nothing can match
//   pipeline of many searches (batch of arg-groups, :3236,3408)   slice_scanner::find_eq_counts(values, n, counts)
//   ... with the matching rows of every search (find_eq(sv,       slice_scanner::find_eq_indices(values, n, offsets, ids)
//        value, bi) :1096 per value)                                  one CSR of ascending row ids for the whole batch
//   find_gt / find_ge / find_lt / find_le / find_range             slice_scanner::find_gt(value, bv_out) ...
//        :1135-1174 -> :2690-2880, find_gt_horizontal_u :2914         ONE pass over the planes (bmx_slice_compare,
//   find_zero :2290, find_nonzero :4464, find_eq(sv, 0, ..) :4366     bmx_kernels4.h) instead of a chain of vector ops
//   a loop of find_range(sv, from, to, bv) :2862 + bv.count()     slice_scanner::find_range_counts(lo, hi, n, counts)
//        (histograms, quantile boundaries, BETWEEN lists)         slice_scanner::histogram(edges, n_edges, counts)
//                                                                    the planes are read once per 8 distinct thresholds,
//                                                                    not once per range (bmx_slice_range_counts, bmx_kernels18.h)
//   sv.gather(buf, idx, n, BM_SORTED_UNIFORM) over the rows of a    slice_scanner::values(rows_mask, values, rows)
//        bit-vector (set2set_11_transform::remap :2170-2204)          one device only (bmx_slice_values, bmx_kernels19.h)
//
// The slices stay resident in HBM; a batch of searches is ONE counts-only pipeline launch (the
// LDS-staged kernel when many groups share the slices).  The container
// (bm::sparse_vector<>) stays on the host: bmx::upload_slices (bm_adapter.hpp) uploads its slices.
#pragma once

#include <vector>

#include "bvector.hpp"

namespace bmx {

/// what the scanner needs from a vector family: its context type and the one-pass comparison entry of the C-ABI
template <class BV> struct scanner_traits;
template <> struct scanner_traits<bvector> {
    typedef context ctx_type;
    typedef bmx_vec handle_type;
    static int compare(ctx_type& c, const handle_type* const* h, size_t n, int pred, uint64_t v0, uint64_t v1, uint64_t size,
                       const handle_type* nn, handle_type** r, uint64_t* cnt)
    { return bmx_slice_compare(c.handle(), h, n, pred, v0, v1, size, nn, r, cnt); }
    static int eq_counts(ctx_type& c, const handle_type* const* h, size_t n, const uint64_t* values, size_t nv, uint64_t size,
                         const handle_type* nn, uint64_t* counts)
    { return bmx_slice_eq_counts(c.handle(), h, n, values, nv, size, nn, counts); }
    static int range_counts(ctx_type& c, const handle_type* const* h, size_t n, const uint64_t* lo, const uint64_t* hi, size_t nr, uint64_t size,
                            const handle_type* nn, uint64_t* counts)
    { return bmx_slice_range_counts(c.handle(), h, n, lo, hi, nr, size, nn, counts); }
    /// (one device only: a group has no twin of this entry)
    static int values(ctx_type& c, const handle_type* const* h, size_t n, uint64_t size, const handle_type* nn, const handle_type* sel,
                      int width, void* values, void* rows, uint64_t cap, uint64_t* cnt)
    { return bmx_slice_values(c.handle(), h, n, size, nn, sel, width, values, rows, cap, cnt); }
};

/// BV = bmx::bvector (one device, `slice_scanner`) or bmx::gbvector (a device group, `gslice_scanner` in group.hpp:
/// planes sharded by block range, every member searches its own rows)
template <class BV>
class basic_slice_scanner {
    typedef scanner_traits<BV> traits;
    typedef typename traits::ctx_type ctx_type;
    typedef BV bvector;                     // (the method bodies below are written against this name)
public:
    typedef uint64_t value_type;
    explicit basic_slice_scanner(ctx_type& ctx) : ctx_(&ctx), agg_(ctx) {}

    /// slice i holds bit i of every element; nullptr = the plane does not exist (sv.get_slice(i) == 0).
    /// slices.size() plays effective_slices(); size = sv.size() (rows; 0 = the longest slice);
    /// not_null = device copy of sv.get_null_bvector() (nullptr: the container has no NULLs).
    void bind(const std::vector<const bvector*>& slices, size_type size = 0, const bvector* not_null = nullptr)
    {
        slices_ = slices; size_ = size; not_null_ = not_null;
        if (!size_) for (size_t i = 0; i < slices_.size(); ++i) if (slices_[i] && slices_[i]->size() > size_) size_ = slices_[i]->size();
    }
    size_t effective_slices() const noexcept { return slices_.size(); }
    size_type size() const noexcept { return size_; }
    /// what bind() was given (read-only): the planes, the not-NULL vector (nullptr: none) and the context
    const std::vector<const bvector*>& slices() const noexcept { return slices_; }
    const bvector* not_null() const noexcept { return (not_null_ && !not_null_->empty_handle()) ? not_null_ : nullptr; }
    ctx_type& ctx() const noexcept { return *ctx_; }

    /// the planes are those of a signed container (slices[0] = the sign, s2u, src/bmbmatrix.h:2536): values() converts the
    /// patterns, set2set_11_transform refuses the column.  The searches above and below take what their comments say.
    void set_signed(bool on) noexcept { signed_ = on; }
    bool is_signed() const noexcept { return signed_; }

    /// the values of the rows of rows_mask (nullptr: every row) that are not NULL and below size(), ascending by row -- what
    /// sv.gather delivers for the rows set2set_11_transform::remap enumerates (src/bmsparsevec_algo.h:2170-2204) -- and, when
    /// rows is given, their row ids (bmx_slice_values).  A signed scanner's patterns are converted to integers (u2s), held as
    /// two's complement in the uint64_t.
    void values(const bvector* rows_mask, std::vector<uint64_t>& values, std::vector<size_type>* rows = nullptr) const
    {
        typedef typename traits::handle_type handle_type;
        std::vector<const handle_type*> h(slices_.size() ? slices_.size() : 1, nullptr);
        for (size_t i = 0; i < slices_.size(); ++i) h[i] = (slices_[i] && !slices_[i]->empty_handle()) ? slices_[i]->handle() : nullptr;
        const handle_type* nn = (not_null_ && !not_null_->empty_handle()) ? not_null_->handle() : nullptr;
        const handle_type* sel = nullptr;
        values.clear(); if (rows) rows->clear();
        if (rows_mask) { if (rows_mask->empty_handle()) return; sel = rows_mask->handle(); }      // (a vector without content selects nothing)
        uint64_t n = 0;
        int rc = traits::values(*ctx_, h.data(), slices_.size(), size_, nn, sel, 8, nullptr, nullptr, 0, &n);   // (the number of rows first)
        if (rc != BMX_OK && !(rc == BMX_ERR_RANGE && n)) check(rc);
        if (!n) return;
        values.resize(n); if (rows) rows->resize(n);
        check(traits::values(*ctx_, h.data(), slices_.size(), size_, nn, sel, 8, values.data(), rows ? rows->data() : nullptr, n, &n));
        if (signed_) for (size_t i = 0; i < values.size(); ++i) { const uint64_t u = values[i]; values[i] = (u & 1u) ? ~(u >> 1) : (u >> 1); }
    }

    // ---- comparison searches (unsigned values): one pass over the planes ----
    void find_gt(uint64_t value, bvector& bv_out) { compare(BMX_CMP_GT, value, 0, &bv_out); }            // :2690
    void find_ge(uint64_t value, bvector& bv_out) { compare(BMX_CMP_GE, value, 0, &bv_out); }            // :2717
    void find_lt(uint64_t value, bvector& bv_out) { compare(BMX_CMP_LT, value, 0, &bv_out); }            // :2790
    void find_le(uint64_t value, bvector& bv_out) { compare(BMX_CMP_LE, value, 0, &bv_out); }            // :2824
    void find_range(uint64_t from, uint64_t to, bvector& bv_out) { compare(BMX_CMP_RANGE, from, to, &bv_out); }   // :2862
    void find_zero(bvector& bv_out) { compare(BMX_CMP_ZERO, 0, 0, &bv_out); }                            // :2290 (null_correct)
    void find_nonzero(bvector& bv_out) { compare(BMX_CMP_NONZERO, 0, 0, &bv_out); }                      // :4464
    /// popcount of a comparison search, nothing materialised (pred = BMX_CMP_*)
    size_type count(int pred, uint64_t v0, uint64_t v1 = 0) { return compare(pred, v0, v1, nullptr); }

    /// rows equal to `value` -> bv_out; false when nothing was found (value 0: find_zero, :4366)
    bool find_eq(uint64_t value, bvector& bv_out)
    {
        if (!value) { compare(BMX_CMP_EQ, 0, 0, &bv_out); return bv_out.any(); }
        typename aggregator<bvector>::arg_groups g;
        if (!add_groups(value, g)) { bv_out.clear(); return false; }
        return agg_.combine_and_sub(bv_out, g.arg_bv0.data(), g.arg_bv0.size(), g.arg_bv1.data(), g.arg_bv1.size(), false);
    }

    /// find_eq(sv, value, bi)  src/bmsparsevec_algo.h:1096: the matching rows as sorted indices fed into a back-insert iterator
    template <class BII, class = decltype(*std::declval<BII&>() = size_type(0))>
    bool find_eq(uint64_t value, BII bi)
    {
        bvector t(*ctx_);
        bool f = find_eq(value, t);
        if (f) t.copy_to(bi);
        return f;
    }

    /// index of the first row equal to `value`
    bool find_first_eq(uint64_t value, size_type& idx)
    {
        if (!value) return false;                                        // :2428
        typename aggregator<bvector>::arg_groups g;
        if (!add_groups(value, g)) return false;
        return agg_.find_first_and_sub(idx, g.arg_bv0.data(), g.arg_bv0.size(), g.arg_bv1.data(), g.arg_bv1.size());
    }

    /// counts[q] = number of rows equal to values[q].  Up to 32 planes: ONE pass over the planes whatever n is
    /// (bmx_slice_eq_counts: bit-matrix transposition + hash lookup); more planes, or use_pipeline: one AND-SUB group
    /// per value in one counts-only pipeline (the reference's formulation, :3236,3408)
    void find_eq_counts(const uint64_t* values, size_t n, uint64_t* counts, bool use_pipeline = false)
    {
        if (!use_pipeline && slices_.size() <= 32) {
            typedef typename traits::handle_type handle_type;
            std::vector<const handle_type*> h(slices_.size() ? slices_.size() : 1, nullptr);
            for (size_t i = 0; i < slices_.size(); ++i) h[i] = slices_[i] ? slices_[i]->handle() : nullptr;
            check(traits::eq_counts(*ctx_, h.data(), slices_.size(), values, n, size_,
                                    (not_null_ && !not_null_->empty_handle()) ? not_null_->handle() : nullptr, counts));
            return;
        }
        typedef typename aggregator<bvector>::template pipeline<agg_opt_only_counts> pipe_t;
        pipe_t pipe(*ctx_);
        std::vector<size_t> slot(n, ~size_t(0));
        for (size_t q = 0; q < n; ++q) {
            counts[q] = 0;
            if (!values[q]) { counts[q] = count(BMX_CMP_EQ, 0); continue; }
            typename aggregator<bvector>::arg_groups g;
            if (!add_groups(values[q], g)) continue;                     // impossible value: count 0
            typename aggregator<bvector>::arg_groups* pg = pipe.add();
            *pg = g;
            slot[q] = pipe.size() - 1;
        }
        if (!pipe.size()) return;
        pipe.complete();
        agg_.combine_and_sub(pipe);
        for (size_t q = 0; q < n; ++q) if (slot[q] != ~size_t(0)) counts[q] = pipe.get_bv_count_vector()[slot[q]];
    }

    /// counts[q] = not-NULL rows with lo[q] <= value <= hi[q] (closed; a reversed pair is swapped, as find_range does, :2862):
    /// a loop of find_range + count() in one pass over the planes per 8 distinct thresholds (bmx_slice_range_counts)
    void find_range_counts(const value_type* lo, const value_type* hi, size_t n, uint64_t* counts)
    {
        typedef typename traits::handle_type handle_type;
        std::vector<const handle_type*> h(slices_.size() ? slices_.size() : 1, nullptr);
        for (size_t i = 0; i < slices_.size(); ++i) h[i] = slices_[i] ? slices_[i]->handle() : nullptr;
        check(traits::range_counts(*ctx_, h.data(), slices_.size(), lo, hi, n, size_,
                                   (not_null_ && !not_null_->empty_handle()) ? not_null_->handle() : nullptr, counts));
    }

    /// n_edges - 1 bins [edges[k], edges[k + 1]) over ascending edges; a bin whose edges are equal is empty (0)
    void histogram(const value_type* edges, size_t n_edges, uint64_t* counts)
    {
        if (n_edges < 2) return;
        std::vector<value_type> lo, hi; std::vector<size_t> bin;
        for (size_t k = 0; k + 1 < n_edges; ++k) {
            if (edges[k + 1] < edges[k]) throw error(BMX_ERR_BADARG, "histogram edges must ascend");
            counts[k] = 0;
            if (edges[k] < edges[k + 1]) { lo.push_back(edges[k]); hi.push_back(edges[k + 1] - 1); bin.push_back(k); }
        }
        std::vector<uint64_t> c(bin.size(), 0);
        if (!bin.empty()) find_range_counts(lo.data(), hi.data(), bin.size(), c.data());
        for (size_t i = 0; i < bin.size(); ++i) counts[bin[i]] = c[i];
    }

    /// a batch of find_eq(sv, value, bi) (:1096): ids[offsets[q] .. offsets[q + 1]) = the rows equal to values[q], ascending.  One
    /// AND-SUB group per value in ONE index-list pipeline run (aggregator::combine_and_sub_indices); a value with a set bit that
    /// has no plane gives an empty segment; value 0 goes through the comparison kernel (find_zero, :4366) and is spliced in here
    void find_eq_indices(const uint64_t* values, size_t n, std::vector<size_type>& offsets, std::vector<size_type>& ids)
    {
        typedef typename aggregator<bvector>::template pipeline<agg_opt_disable_bvects_and_counts> pipe_t;
        pipe_t pipe(*ctx_);
        std::vector<size_t> slot(n, ~size_t(0));
        bool any_zero = false;
        for (size_t q = 0; q < n; ++q) {
            if (!values[q]) { any_zero = true; continue; }
            typename aggregator<bvector>::arg_groups g;
            if (!add_groups(values[q], g)) continue;                     // impossible value: empty segment
            *pipe.add() = g;
            slot[q] = pipe.size() - 1;
        }
        std::vector<size_type> poff(1, 0), pids, zero;
        if (pipe.size()) { pipe.complete(); agg_.combine_and_sub_indices(pipe, poff, pids); }
        if (any_zero) { bvector z(*ctx_); compare(BMX_CMP_EQ, 0, 0, &z); z.to_indices(zero); }
        offsets.assign(n + 1, 0); ids.clear();
        if (!any_zero && pipe.size() == n) { ids.swap(pids); offsets = poff; return; }       // every value has its own group: no splice
        for (size_t q = 0; q < n; ++q) {
            if (!values[q]) ids.insert(ids.end(), zero.begin(), zero.end());
            else if (slot[q] != ~size_t(0)) ids.insert(ids.end(), pids.begin() + (ptrdiff_t)poff[slot[q]], pids.begin() + (ptrdiff_t)poff[slot[q] + 1]);
            offsets[q + 1] = ids.size();
        }
    }

private:
    size_type compare(int pred, uint64_t v0, uint64_t v1, bvector* out)
    {
        typedef typename traits::handle_type handle_type;
        std::vector<const handle_type*> h(slices_.size() ? slices_.size() : 1, nullptr);
        for (size_t i = 0; i < slices_.size(); ++i) h[i] = slices_[i] ? slices_[i]->handle() : nullptr;
        handle_type* r = nullptr; uint64_t c = 0;
        check(traits::compare(*ctx_, h.data(), slices_.size(), pred, v0, v1, size_,
                              (not_null_ && !not_null_->empty_handle()) ? not_null_->handle() : nullptr,
                              out ? &r : nullptr, out ? nullptr : &c));
        if (out) out->adopt(r);
        return c;
    }
    // prepare_and_sub_aggregator (src/bmsparsevec_algo.h:2593-2640)
    bool add_groups(uint64_t value, typename aggregator<bvector>::arg_groups& g) const
    {
        for (int bit = 63; bit >= 0; --bit) {                            // backward order (:2614)
            if (!((value >> bit) & 1u)) continue;
            if ((size_t)bit >= slices_.size() || !slices_[(size_t)bit]) return false;      // :2621
            g.add(slices_[(size_t)bit], 0);
        }
        for (size_t i = 0; i < slices_.size(); ++i)
            if (slices_[i] && (i >= 64 || !((value >> i) & 1u))) g.add(slices_[i], 1);  // :2626-2631
        return true;
    }

    ctx_type* ctx_;
    aggregator<bvector> agg_;
    std::vector<const bvector*> slices_;
    size_type size_ = 0;
    const bvector* not_null_ = nullptr;
    bool signed_ = false;
};

typedef basic_slice_scanner<bvector> slice_scanner;

} // namespace bmx
