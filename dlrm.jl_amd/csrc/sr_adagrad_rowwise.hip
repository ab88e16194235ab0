// sr_adagrad_rowwise.hip — the row-wise Adagrad embedding update on bf16 tables with a stochastically rounded store
// (gfx950): the rule that fits the largest table sets (one fp32 word per row beside the bf16 rows).
//
// The apply launch of update.hip (apply_kernel.hpp) with apply.hpp's StochasticRowwiseAdagrad rule at its write
// sites: the row-wise rule's G, state word and fp32 result W', exactly as adagrad_rowwise.hip computes them (the sum
// over c in that unit's fixed order per site),
//   m[r] += (1/D) sum_c G[c]^2;  W' = w[r][c] - lr G[c] / (sqrt(m[r]) + eps);  w[r][c] = sr_bf16(W', R)
// with R = 16 Philox4x32-10 bits of (seed, step, table, row, column), sr_sgd.hip's definition unchanged.  The state
// word is written with the bits adagrad_rowwise.hip writes.  Only bf16 tables are instantiated, MODE 0 and 1; the
// step word is read and advanced as in sr_adagrad.hip.
#include "apply_kernel.hpp"

namespace dlrm {

// (tdtype: bf16, the caller checked; r.state: the device array of per-table fp32 [nrows] state pointers)
int launch_sr_rowwise_adagrad_apply(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, int T_, int D,
                                    int, int L, int64_t N, const void* grad, int gdtype, int64_t grad_ld,
                                    int64_t grad_offset, const BoundRule& r, const SinglesArgs& sa, const PrepArgs*) {
    if (T_ == 0 || N == 0) return DLRM_OK;  // (nothing launched: the step stays)
    const int rc = launch_apply_rule(ctx, ix, tabs, aligned16, T_, D, DLRM_BF16, L, N, grad, gdtype, grad_ld, grad_offset,
                                     StochasticRowwiseAdagrad{{r.lr, r.eps, (float* const*)r.state},
                                                              {(uint32_t)r.seed, (uint32_t)(r.seed >> 32), r.step, 0u, 0u}},
                                     sa, nullptr);
    if (rc) return rc;
    return launch_sr_step_advance(ctx, r.step);
}

}  // namespace dlrm
