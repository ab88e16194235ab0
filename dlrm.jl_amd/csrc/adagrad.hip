// adagrad.hip — EmbeddingTables.update!(ADAGrad(lr, eps), ...) on gfx950: the element-wise rule.
//
// The apply launch of update.hip (apply_kernel.hpp: one write per touched row, the row's whole
// gradient sum G in hand at the write) with apply.hpp's Adagrad rule at its write sites:
//   A[r][c] += G[c]^2;  w[r][c] -= lr G[c] / (sqrt(A[r][c]) + eps)
// A row's fp32 state row is loaded where its table row is and written once with it.
#include "apply_kernel.hpp"

namespace dlrm {
template ApplyFn launch_rule_apply<Adagrad>;
}  // namespace dlrm
