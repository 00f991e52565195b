// imm3_merge_view_host.cpp -- a view of merged groups on the HOST (imm3_merge_view_plan.h: merge_view_host): filter, then order, then
// limit over records, by the key builder and the evaluator the kernels of imm3_merge_view.hip run.  No HIP call: the single-process
// flavour (imm3_comm_merge_groups_view_all) finishes here behind its host combine, the device flavour answers an empty list here, and
// tests/native/merge_view_asan.cpp drives it alone.
#include "imm3_merge_view_plan.h"

#include <algorithm>
#include <array>
#include <vector>

namespace imm3 {

void merge_view_host(const MergeViewPlan &p, const unsigned long long *recs, size_t n, uint32_t *order_out, size_t *n_out, size_t *n_kept) {
    struct Keyed {
        std::array<uint32_t, 4> k;
        uint32_t idx;
    };
    std::vector<Keyed> kept;
    kept.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        const unsigned long long *rec = recs + i * (size_t)p.rec_words;
        if (!merge_view_keep(p, rec)) continue;
        Keyed e;
        merge_view_key(p, rec, e.k.data());
        e.idx = (uint32_t)i;
        kept.push_back(e);
    }
    // (the tie makes every key unique as long as no two records share `first`: any sort gives the same list)
    std::sort(kept.begin(), kept.end(), [](const Keyed &x, const Keyed &y) { return x.k != y.k ? x.k < y.k : x.idx < y.idx; });
    const size_t out = p.limit > 0 && (unsigned long long)p.limit < (unsigned long long)kept.size() ? (size_t)p.limit : kept.size();
    for (size_t i = 0; i < out; ++i) order_out[i] = kept[i].idx;
    *n_out = out;
    *n_kept = kept.size();
}

} // namespace imm3
