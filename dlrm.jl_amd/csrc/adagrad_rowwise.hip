// adagrad_rowwise.hip — the row-wise Adagrad embedding update on gfx950.
//
// The apply launch of update.hip (apply_kernel.hpp) with apply.hpp's RowwiseAdagrad rule at its
// write sites: one fp32 word per table row,
//   m[r] += (1/D) sum_c G[c]^2;  w[r][c] -= lr G[c] / (sqrt(m[r]) + eps)
// The sum over c has a fixed order per site (apply.hpp), so the result is bitwise reproducible.
#include "apply_kernel.hpp"

namespace dlrm {

// (r.state: the device array of per-table fp32 [nrows] state pointers)
int launch_rowwise_adagrad_apply(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, int T_, int D,
                                 int tdtype, int L, int64_t N, const void* grad, int gdtype, int64_t grad_ld,
                                 int64_t grad_offset, const BoundRule& r, const SinglesArgs& sa, const PrepArgs*) {
    return launch_apply_rule(ctx, ix, tabs, aligned16, T_, D, tdtype, L, N, grad, gdtype, grad_ld, grad_offset,
                             RowwiseAdagrad{r.lr, r.eps, (float* const*)r.state}, sa, nullptr);
}

}  // namespace dlrm
