// split_step.hip — the apply launch of the training step on split-bf16 tables (gfx950) when it carries the next
// batch's split indexer build (dlrm_split_step_bwd_prepare): apply_step.hpp with apply.hpp's SplitDescent rule.
// Only bf16 tables and the step's fp32 dt rows are instantiated.  MODE 0 and 1 stay in split_sgd.hip.
#include "apply_step.hpp"

namespace dlrm {

int launch_split_step_apply(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, int T_, int D, int,
                            int, int64_t N, const void* dt, int, int64_t dt_ld, int64_t dt_offset, const BoundRule& r,
                            const SinglesArgs& sa, const PrepArgs* pa) {
    return launch_step_apply_rule(ctx, ix, tabs, aligned16, T_, D, DLRM_BF16, N, (const float*)dt, dt_ld, dt_offset,
                                  SplitDescent{r.lr, (uint16_t* const*)r.state}, sa, pa, [&](const SinglesArgs& s1) {
                                      return launch_split_sgd_apply(ctx, ix, tabs, aligned16, T_, D, DLRM_BF16, 1, N, dt,
                                                                    DLRM_F32, dt_ld, dt_offset, r, s1, nullptr);
                                  });
}

}  // namespace dlrm
