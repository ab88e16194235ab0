// adagrad_rowwise.hip — the row-wise Adagrad embedding update on gfx950.
//
// The apply launch of update.hip (apply_kernel.hpp) with apply.hpp's RowwiseAdagrad rule at its
// write sites: one fp32 word per table row,
//   m[r] += (1/D) sum_c G[c]^2;  w[r][c] -= lr G[c] / (sqrt(m[r]) + eps)
// The sum over c has a fixed order per site (apply.hpp), so the result is bitwise reproducible.
#include "apply_kernel.hpp"

namespace dlrm {
template ApplyFn launch_rule_apply<RowwiseAdagrad>;
}  // namespace dlrm
