// sr_adagrad_step.hip — the apply launch of the training step with the element-wise Adagrad rule and the stochastic
// store on bf16 tables (gfx950) when it carries the next batch's split indexer build
// (dlrm_sr_adagrad_step_bwd_prepare): apply_step.hpp (apply_kernel.hpp in MODE 2 / 3 / 5) with apply.hpp's
// StochasticAdagrad rule at its write sites.  Only bf16 tables and the step's fp32 dt rows are instantiated.  MODE 0
// and 1 stay in sr_adagrad.hip.
//
// The step word is sr_step.hip's: the backward launch and this launch of one training step read the same value, and
// the one-thread advance follows the launch that ran the apply.  launch_sr_adagrad_apply (the route with once-hit
// items or without a vector kernel) ends with it itself.
#include "apply_step.hpp"

namespace dlrm {

int launch_sr_adagrad_step_apply(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, int T_, int D,
                                 int, int, int64_t N, const void* dt, int, int64_t dt_ld, int64_t dt_offset,
                                 const BoundRule& r, const SinglesArgs& sa, const PrepArgs* pa) {
    const StochasticAdagrad rule{{r.lr, r.eps, (float* const*)r.state},
                                 {(uint32_t)r.seed, (uint32_t)(r.seed >> 32), r.step, 0u, 0u}};
    bool advanced = false;  // by launch_sr_adagrad_apply (nothing to launch: it leaves the word alone)
    const int rc = launch_step_apply_rule(ctx, ix, tabs, aligned16, T_, D, DLRM_BF16, N, (const float*)dt, dt_ld,
                                          dt_offset, rule, sa, pa, [&](const SinglesArgs& s) {
                                              advanced = true;
                                              return launch_sr_adagrad_apply(ctx, ix, tabs, aligned16, T_, D, DLRM_BF16,
                                                                             1, N, dt, DLRM_F32, dt_ld, dt_offset, r, s,
                                                                             nullptr);
                                          });
    if (rc || advanced) return rc;
    return launch_sr_step_advance(ctx, r.step);
}

}  // namespace dlrm
