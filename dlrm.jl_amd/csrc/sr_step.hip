// sr_step.hip — the apply launch of the training step with the stochastic rule on bf16 tables (gfx950) when it
// carries the next batch's split indexer build (dlrm_sr_step_bwd_prepare), and the advance of the step word that
// ends every such step.
//
// apply_step.hpp's launch (apply_kernel.hpp in MODE 2 / 3 / 5: the build's workgroups first, then chunks and hot
// slices; no once-hit items: the step backward stepped those rows) with apply.hpp's StochasticDescent rule at its
// write sites.  Only bf16 tables and the step's fp32 dt rows are instantiated.  MODE 0 and 1 stay in sr_sgd.hip;
// the two units compile beside update.hip.
//
// The step word: the backward launch and this launch of one training step read the same value (every workgroup
// once, StochasticDescent::load_step); the one-thread advance follows the launch that ran the apply, in stream
// order.  launch_sr_sgd_apply (the route with once-hit items or without a vector kernel) ends with it itself.
#include "apply_step.hpp"

namespace dlrm {

int launch_sr_step_apply(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, int T_, int D, int, int,
                         int64_t N, const void* dt, int, int64_t dt_ld, int64_t dt_offset, const BoundRule& r,
                         const SinglesArgs& sa, const PrepArgs* pa) {
    const StochasticDescent rule{r.lr, (uint32_t)r.seed, (uint32_t)(r.seed >> 32), r.step, 0u, 0u};
    bool advanced = false;  // by launch_sr_sgd_apply (nothing to launch: it leaves the word alone)
    const int rc = launch_step_apply_rule(ctx, ix, tabs, aligned16, T_, D, DLRM_BF16, N, (const float*)dt, dt_ld,
                                          dt_offset, rule, sa, pa, [&](const SinglesArgs& s) {
                                              advanced = true;
                                              return launch_sr_sgd_apply(ctx, ix, tabs, aligned16, T_, D, DLRM_BF16, 1, N,
                                                                         dt, DLRM_F32, dt_ld, dt_offset, r, s, nullptr);
                                          });
    if (rc || advanced) return rc;
    return launch_sr_step_advance(ctx, r.step);
}

}  // namespace dlrm
