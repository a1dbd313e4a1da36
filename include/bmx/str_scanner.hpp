// bmx/str_scanner.hpp -- string search over the device-resident planes of a bm::str_sparse_vector<>: the find_eq_str half of
// bm::sparse_vector_scanner<SV> (src/bmsparsevec_algo.h), header-only over bmx.h and bvector.hpp.
//
//   reference                                                     here
//   ------------------------------------------------------------  ----------------------------------
//   find_eq_str(sv, str, bv_out)  :1194                           str_scanner::find_eq_str(str, bv_out)
//   find_eq_str(sv, str, pos)     :1208                           str_scanner::find_eq_str(str, pos)
//   find_eq_str_prefix(sv, str, bv_out) :1221                     str_scanner::find_eq_str_prefix(str, bv_out)
//   prepare_and_sub_aggregator(sv, str, octet_start, prefix_sub)  str_scanner::add_groups()  (the one place groups are built)
//        :2546-2588: octets in reverse order, per octet the set bits into AND and the clear bits that have a plane into SUB
//        (add_agg_char :1817), a set bit without a plane => nothing can match (:2569); with prefix_sub every plane above the
//        string's length into SUB (:2575-2586)
//   find_eq_str(pipe) :3263 (a batch of strings as one pipeline)  str_scanner::find_eq_str_counts / find_eq_str_first /
//                                                                    find_eq_str_indices
//   remap_tosv / remap_matrix2_ (src/bmstrsparsevec.h:1583)       str_scanner::set_remap(tables, octets)
//
// Plane octet * 8 + bit holds bit `bit` of character `octet` of every row (src/bmstrsparsevec.h:1423).  A batch of BATCH_MIN
// strings or more goes through bmx_slice_eq_keys: ONE pass over the planes for the whole batch (bmx_kernels20.h) where the
// pipeline reads the planes of every group; shorter batches, use_pipeline, or more than BMX_EQK_MAX_PLANES planes: one AND-SUB
// group per string.
// Not here: bfind_eq_str / lower_bound_str (binary search over a sorted vector) and rank-select-compressed string vectors (the
// reference does not search those either, :3382-3386).
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "bvector.hpp"

namespace bmx {

class str_scanner {
public:
    /// batches of at least this many strings take the batch entry (TUNING.md "str_scanner": the measured crossover)
    static constexpr size_t BATCH_MIN = 64;

    explicit str_scanner(context& ctx) : ctx_(&ctx), agg_(ctx), rows_(ctx) {}

    /// planes[p] = device vector of plane p (nullptr: the plane does not exist); planes.size() plays rows_not_null() of the
    /// bit matrix; size = sv.size(); not_null = device copy of sv.get_null_bvector() (nullptr: no NULLs)
    void bind(const std::vector<const bvector*>& planes, size_type size, const bvector* not_null = nullptr)
    {
        planes_ = planes; size_ = size; not_null_ = (not_null && !not_null->empty_handle()) ? not_null : nullptr;
        rows_.clear(); longer_ = false;
        for (size_t i = 0; i < planes_.size(); ++i) {
            if (planes_[i] && planes_[i]->empty_handle()) planes_[i] = nullptr;
            if (planes_[i] && planes_[i]->size() > size_) longer_ = true;      // planes that run past size: the rows join the AND lists
        }
    }
    size_type size() const noexcept { return size_; }
    const std::vector<const bvector*>& planes() const noexcept { return planes_; }

    /// one 256-entry code table per octet position (sv.get_remap_matrix(): remap_matrix2_); a character mapped to 0 is in no row
    /// at that position: the string is found nowhere (remap_tosv returning false, :3394-3396).  nullptr: no remap
    void set_remap(const uint8_t* tables, size_t octets)
    {
        if (tables) remap_.assign(tables, tables + octets * 256u); else remap_.clear();
        remap_octets_ = tables ? octets : 0;
    }

    /// rows equal to str -> bv_out; false when nothing was found
    bool find_eq_str(const char* str, bvector& bv_out)
    {
        aggregator<bvector>::arg_groups g;
        if (!add_groups(str, true, g)) { bv_out.clear(); return false; }
        return agg_.combine_and_sub(bv_out, g.arg_bv0.data(), g.arg_bv0.size(), g.arg_bv1.data(), g.arg_bv1.size(), false);
    }
    /// rows that start with str -> bv_out
    bool find_eq_str_prefix(const char* str, bvector& bv_out)
    {
        aggregator<bvector>::arg_groups g;
        if (!add_groups(str, false, g)) { bv_out.clear(); return false; }
        return agg_.combine_and_sub(bv_out, g.arg_bv0.data(), g.arg_bv0.size(), g.arg_bv1.data(), g.arg_bv1.size(), false);
    }
    /// the lowest row equal to str
    bool find_eq_str(const char* str, size_type& pos)
    {
        aggregator<bvector>::arg_groups g;
        if (!add_groups(str, true, g)) return false;
        return agg_.find_first_and_sub(pos, g.arg_bv0.data(), g.arg_bv0.size(), g.arg_bv1.data(), g.arg_bv1.size());
    }

    /// counts[q] = rows equal to strs[q]: the batch entry, or one counts pipeline (the reference's find_eq_str(pipe), :3263)
    void find_eq_str_counts(const std::vector<std::string>& strs, std::vector<uint64_t>& counts, bool use_pipeline = false)
    {
        const size_t n = strs.size();
        counts.assign(n, 0);
        if (!n) return;
        if (use_batch(n, use_pipeline)) { eq_keys(strs, counts.data(), nullptr, nullptr); return; }
        typedef aggregator<bvector>::pipeline<agg_opt_only_counts> pipe_t;
        pipe_t pipe(*ctx_);
        std::vector<size_t> slot(n, ~size_t(0));
        for (size_t q = 0; q < n; ++q) {
            aggregator<bvector>::arg_groups g;
            if (!add_groups(strs[q].c_str(), true, g)) continue;
            *pipe.add() = g;
            slot[q] = pipe.size() - 1;
        }
        if (!pipe.size()) return;
        pipe.complete();
        agg_.combine_and_sub(pipe);
        for (size_t q = 0; q < n; ++q) if (slot[q] != ~size_t(0)) counts[q] = pipe.get_bv_count_vector()[slot[q]];
    }

    /// pos[q] = the lowest row equal to strs[q] where found[q] != 0 (else 0)
    void find_eq_str_first(const std::vector<std::string>& strs, std::vector<size_type>& pos, std::vector<uint8_t>& found, bool use_pipeline = false)
    {
        const size_t n = strs.size();
        pos.assign(n, 0); found.assign(n, 0);
        if (!n) return;
        if (use_batch(n, use_pipeline)) { eq_keys(strs, nullptr, pos.data(), found.data()); return; }
        for (size_t q = 0; q < n; ++q) { size_type p = 0; if (find_eq_str(strs[q].c_str(), p)) { pos[q] = p; found[q] = 1; } }
    }

    /// ids[offsets[q] .. offsets[q + 1]) = the rows equal to strs[q], ascending: one index-list pipeline run for the batch
    void find_eq_str_indices(const std::vector<std::string>& strs, std::vector<size_type>& offsets, std::vector<size_type>& ids)
    {
        const size_t n = strs.size();
        typedef aggregator<bvector>::pipeline<agg_opt_disable_bvects_and_counts> pipe_t;
        pipe_t pipe(*ctx_);
        std::vector<size_t> slot(n, ~size_t(0));
        for (size_t q = 0; q < n; ++q) {
            aggregator<bvector>::arg_groups g;
            if (!add_groups(strs[q].c_str(), true, g)) continue;
            *pipe.add() = g;
            slot[q] = pipe.size() - 1;
        }
        std::vector<size_type> poff(1, 0), pids;
        if (pipe.size()) { pipe.complete(); agg_.combine_and_sub_indices(pipe, poff, pids); }
        offsets.assign(n + 1, 0); ids.clear();
        if (pipe.size() == n) { ids.swap(pids); offsets = poff; return; }
        for (size_t q = 0; q < n; ++q) {
            if (slot[q] != ~size_t(0)) ids.insert(ids.end(), pids.begin() + (ptrdiff_t)poff[slot[q]], pids.begin() + (ptrdiff_t)poff[slot[q] + 1]);
            offsets[q + 1] = ids.size();
        }
    }

private:
    bool use_batch(size_t n, bool use_pipeline) const noexcept
    { return !use_pipeline && planes_.size() <= BMX_EQK_MAX_PLANES && n >= BATCH_MIN; }

    /// the characters the planes hold for str: false = not representable (nothing matches)
    bool code(const char* str, std::string& out) const
    {
        out.assign(str ? str : "");
        if (remap_.empty()) return true;
        if (out.size() > remap_octets_) return false;
        for (size_t i = 0; i < out.size(); ++i) {
            const uint8_t c = remap_[i * 256u + (uint8_t)out[i]];
            if (!c) return false;
            out[i] = (char)c;
        }
        return true;
    }

    /// [0, size): what bounds a search to the column's rows
    const bvector* rows()
    {
        if (rows_.empty_handle() && size_) { std::pair<size_type, size_type> r(0, size_ - 1); rows_.assign_ranges(&r, 1, size_); }
        return &rows_;
    }

    // prepare_and_sub_aggregator (src/bmsparsevec_algo.h:2546-2588); the empty string is find_zero with null correction
    // (:3412-3415): AND = [0, size) and the not-NULL vector, SUB = every plane
    bool add_groups(const char* str, bool prefix_sub, aggregator<bvector>::arg_groups& g)
    {
        std::string s;
        if (!code(str, s) || !size_) return false;
        const size_t len = s.size(), np = planes_.size();
        if (!len) {
            g.add(rows(), 0);
            if (prefix_sub) { g.add(not_null_, 0); for (size_t p = 0; p < np; ++p) g.add(planes_[p], 1); }
            return true;
        }
        for (size_t octet = len; octet-- > 0;) {                          // reverse order (:2559)
            const unsigned value = (uint8_t)s[octet];
            unsigned mask = 0;
            for (unsigned b = 0; b < 8; ++b) if (octet * 8 + b < np && planes_[octet * 8 + b]) mask |= 1u << b;
            if ((value & mask) != value) return false;                    // :2569
            for (unsigned b = 0; b < 8; ++b) if ((value >> b) & 1u) g.add(planes_[octet * 8 + b], 0);
            for (unsigned b = 0; b < 8; ++b) if (((value ^ 0xFFu) & mask) >> b & 1u) g.add(planes_[octet * 8 + b], 1);
        }
        if (prefix_sub) for (size_t p = len * 8; p < np; ++p) g.add(planes_[p], 1);      // :2575-2586
        if (longer_) g.add(rows(), 0);
        return true;
    }

    void eq_keys(const std::vector<std::string>& strs, uint64_t* counts, size_type* first, uint8_t* found)
    {
        const size_t n = strs.size();
        std::vector<std::string> codes(n); std::vector<uint8_t> ok(n, 0);
        size_t kb = (planes_.size() + 7) / 8;
        for (size_t q = 0; q < n; ++q) { ok[q] = code(strs[q].c_str(), codes[q]) ? 1 : 0; if (ok[q] && codes[q].size() > kb) kb = codes[q].size(); }
        kb += 1;                                                          // one octet more than the column: an unrepresentable string's mark
        std::vector<uint8_t> keys(n * kb, 0);
        for (size_t q = 0; q < n; ++q) {
            if (!ok[q]) keys[q * kb + kb - 1] = 1;                        // a bit no plane holds: matches nothing
            else if (!codes[q].empty()) std::memcpy(&keys[q * kb], codes[q].data(), codes[q].size());
        }
        std::vector<const bmx_vec*> h(planes_.size() ? planes_.size() : 1, nullptr);
        for (size_t i = 0; i < planes_.size(); ++i) h[i] = planes_[i] ? planes_[i]->handle() : nullptr;
        check(bmx_slice_eq_keys(ctx_->handle(), h.data(), planes_.size(), size_, not_null_ ? not_null_->handle() : nullptr,
                                keys.data(), kb, n, counts, first, found));
    }

    context* ctx_;
    aggregator<bvector> agg_;
    bvector rows_;
    std::vector<const bvector*> planes_;
    size_type size_ = 0;
    const bvector* not_null_ = nullptr;
    bool longer_ = false;
    std::vector<uint8_t> remap_;
    size_t remap_octets_ = 0;
};

} // namespace bmx
