// sr_adagrad.hip — update!(ADAGrad(lr, eps), ...) on bf16 tables with a stochastically rounded store (gfx950).
//
// The apply launch of update.hip (apply_kernel.hpp) with apply.hpp's StochasticAdagrad rule at its write sites: the
// element-wise rule's G, state update and fp32 result W', exactly as adagrad.hip computes them,
//   A[r][c] += G[c]^2;  W' = w[r][c] - lr G[c] / (sqrt(A[r][c]) + eps);  w[r][c] = sr_bf16(W', R)
// with R = 16 Philox4x32-10 bits of (seed, step, table, row, column), sr_sgd.hip's definition unchanged.  The fp32
// state row is written with the bits adagrad.hip writes: the rounding is of the weights only.  Only bf16 tables
// (TT = uint16_t) are instantiated, MODE 0 and 1.  The step is the device word of the dlrm_adagrad handle made by
// dlrm_adagrad_create_sr: every launch of a call reads it, and sr_sgd.hip's one-thread launch after the call's last
// adds one, in stream order.
#include "apply_kernel.hpp"

namespace dlrm {

// (tdtype: bf16, the caller checked; r.state: the device array of per-table fp32 [nrows][D] state pointers)
int launch_sr_adagrad_apply(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, int T_, int D, int,
                            int L, int64_t N, const void* grad, int gdtype, int64_t grad_ld, int64_t grad_offset,
                            const BoundRule& r, const SinglesArgs& sa, const PrepArgs*) {
    if (T_ == 0 || N == 0) return DLRM_OK;  // (nothing launched: the step stays)
    const int rc = launch_apply_rule(ctx, ix, tabs, aligned16, T_, D, DLRM_BF16, L, N, grad, gdtype, grad_ld, grad_offset,
                                     StochasticAdagrad{{r.lr, r.eps, (float* const*)r.state},
                                                       {(uint32_t)r.seed, (uint32_t)(r.seed >> 32), r.step, 0u, 0u}},
                                     sa, nullptr);
    if (rc) return rc;
    return launch_sr_step_advance(ctx, r.step);
}

}  // namespace dlrm
