// bmx/similarity.hpp -- similarity batches over device vectors (the interface of src/bmalgo_similarity.h).
//
//   bm::similarity_descriptor<SO, DMD_SZ, IDX_VALUE, SValue, SFunc>   bmx::similarity_descriptor (same parameters)
//   bm::similarity_batch<SDESCR>::calculate / sort                    bmx::similarity_batch<SDESCR>
//   bm::build_jaccard_similarity_batch(sbatch, sv)                    bmx::build_jaccard_similarity_batch(sbatch, slices)
//
// The difference is in calculate(): the reference runs distance_operation once per descriptor; here the batch collects its
// distinct objects and issues ONE all-pairs matrix call over them (bmx_distance_matrix, symmetric), then every descriptor
// adds its metrics from that matrix and the functor reduces them on the host.  The bit-sliced sparse vector stays with the
// host library, so the Jaccard batch is built from its slices (`slices[i]` = plane i, null where the plane is absent).
#pragma once

#include <algorithm>
#include <cstddef>
#include <functional>
#include <unordered_map>
#include <vector>

#include "bvector.hpp"

namespace bmx {

/// two objects, their indexes, DMD_SZ distance metrics and the similarity the functor made of them
template <typename SO, unsigned DMD_SZ, typename IDX_VALUE, typename SValue, typename SFunc>
class similarity_descriptor {
public:
    typedef SO similarity_object_type;
    typedef SValue similarity_value_type;
    typedef SFunc similarity_functor;

    similarity_descriptor() : similarity_(), so1_(nullptr), so2_(nullptr), so1_idx_(), so2_idx_() {}
    similarity_descriptor(const SO* so1, const SO* so2, const distance_metric_descriptor* dmd)
        : similarity_(), so1_(so1), so2_(so2), so1_idx_(), so2_idx_() { set_metrics(dmd); }
    similarity_descriptor(const SO* so1, IDX_VALUE i1, const SO* so2, IDX_VALUE i2, const distance_metric_descriptor* dmd)
        : similarity_(), so1_(so1), so2_(so2), so1_idx_(i1), so2_idx_(i2) { set_metrics(dmd); }

    bool operator>(const similarity_descriptor& o) const { return similarity_ > o.similarity_; }
    SValue similarity() const { return similarity_; }
    void set_similarity(SValue s) { similarity_ = s; }
    const SO* get_first() const { return so1_; }
    const SO* get_second() const { return so2_; }
    IDX_VALUE get_first_idx() const { return so1_idx_; }
    IDX_VALUE get_second_idx() const { return so2_idx_; }
    distance_metric_descriptor* distance_begin() { return dmd_; }
    distance_metric_descriptor* distance_end() { return dmd_ + DMD_SZ; }
    void set_metric(size_t i, distance_metric m) { dmd_[i].metric = m; }

private:
    void set_metrics(const distance_metric_descriptor* dmd) { for (unsigned i = 0; i < DMD_SZ; ++i) dmd_[i] = dmd[i]; }
    SValue similarity_;
    const SO* so1_;
    const SO* so2_;
    IDX_VALUE so1_idx_, so2_idx_;
    distance_metric_descriptor dmd_[DMD_SZ];
};

/// a batch of descriptors measured together
template <class SDESCR>
struct similarity_batch {
    typedef SDESCR similaruty_descriptor_type;          // (the reference's spelling)
    typedef SDESCR similarity_descriptor_type;
    typedef typename SDESCR::similarity_object_type similarity_object_type;
    typedef typename SDESCR::similarity_value_type similarity_value_type;
    typedef typename SDESCR::similarity_functor similarity_functor;
    typedef std::vector<SDESCR> vector_type;

    /// every descriptor's metrics (added to its results, as distance_operation does) and its similarity, from ONE symmetric
    /// matrix call over the distinct objects of the batch
    void calculate()
    {
        std::vector<const similarity_object_type*> objs;
        std::unordered_map<const similarity_object_type*, size_t> index;
        auto idx = [&](const similarity_object_type* o) {
            auto it = index.find(o);
            if (it != index.end()) return it->second;
            index.emplace(o, objs.size());
            objs.push_back(o);
            return objs.size() - 1;
        };
        std::vector<std::pair<size_t, size_t>> at(descr_vect_.size());
        for (size_t k = 0; k < descr_vect_.size(); ++k)
            at[k] = std::make_pair(idx(descr_vect_[k].get_first()), idx(descr_vect_[k].get_second()));
        const size_t n = objs.size();
        const std::vector<uint64_t> m = n ? distance_matrix(objs, {COUNT_AND, COUNT_A}) : std::vector<uint64_t>();
        for (size_t k = 0; k < descr_vect_.size(); ++k) {
            SDESCR& d = descr_vect_[k];
            const size_t i = at[k].first, j = at[k].second;
            const size_type ab = m[i * n + j], a = m[n * n + i * n + j], b = m[n * n + j * n + i];
            for (distance_metric_descriptor* it = d.distance_begin(); it != d.distance_end(); ++it)
                it->result += detail::metric_value(it->metric, ab, a, b);
            similarity_functor f;
            d.set_similarity(f(d.distance_begin(), d.distance_end()));
        }
    }
    void sort() { std::sort(descr_vect_.begin(), descr_vect_.end(), std::greater<SDESCR>()); }
    void reserve(size_t cap) { descr_vect_.reserve(cap); }
    void push_back(const SDESCR& d) { descr_vect_.push_back(d); }
    size_t size() const { return descr_vect_.size(); }

    std::vector<SDESCR> descr_vect_;
};

/// the triangular Jaccard batch of a bit-sliced vector's planes: a descriptor (COUNT_AND, COUNT_OR) for every pair i < j of
/// present, distinct slices
template <class SIMBATCH>
void build_jaccard_similarity_batch(SIMBATCH& sbatch, const std::vector<const bvector*>& slices)
{
    typedef typename SIMBATCH::similarity_descriptor_type descr;
    const size_t planes = slices.size();
    sbatch.reserve(sbatch.size() + planes * planes / 2);
    distance_metric_descriptor dmd[2] = {distance_metric_descriptor(COUNT_AND), distance_metric_descriptor(COUNT_OR)};
    for (size_t i = 0; i < planes; ++i) {
        const bvector* a = slices[i];
        if (!a) continue;
        for (size_t j = i + 1; j < planes; ++j) {
            const bvector* b = slices[j];
            if (b && b != a) sbatch.push_back(descr(a, (unsigned)i, b, (unsigned)j, dmd));
        }
    }
}

} // namespace bmx
