// adagrad.hip — EmbeddingTables.update!(ADAGrad(lr, eps), ...) on gfx950: the element-wise rule.
//
// The apply launch of update.hip (apply_kernel.hpp: one write per touched row, the row's whole
// gradient sum G in hand at the write) with apply.hpp's Adagrad rule at its write sites:
//   A[r][c] += G[c]^2;  w[r][c] -= lr G[c] / (sqrt(A[r][c]) + eps)
// A row's fp32 state row is loaded where its table row is and written once with it.
#include "apply_kernel.hpp"

namespace dlrm {

// (r.state: the device array of per-table fp32 [nrows][D] state pointers)
int launch_adagrad_apply(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, int T_, int D, int tdtype,
                         int L, int64_t N, const void* grad, int gdtype, int64_t grad_ld, int64_t grad_offset,
                         const BoundRule& r, const SinglesArgs& sa, const PrepArgs*) {
    return launch_apply_rule(ctx, ix, tabs, aligned16, T_, D, tdtype, L, N, grad, gdtype, grad_ld, grad_offset,
                             Adagrad{r.lr, r.eps, (float* const*)r.state}, sa, nullptr);
}

}  // namespace dlrm
