// adagrad_step.hip — the apply launch of the training step with the element-wise Adagrad rule (gfx950) when it
// carries the next batch's split indexer build (dlrm_adagrad_step_bwd_prepare): apply_step.hpp with apply.hpp's
// Adagrad rule.  MODE 0 and 1 stay in adagrad.hip.
#include "apply_step.hpp"

namespace dlrm {

int launch_adagrad_step_apply(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, int T_, int D,
                              int tdtype, int, int64_t N, const void* dt, int, int64_t dt_ld, int64_t dt_offset,
                              const BoundRule& r, const SinglesArgs& sa, const PrepArgs* pa) {
    return launch_step_apply_rule(ctx, ix, tabs, aligned16, T_, D, tdtype, N, (const float*)dt, dt_ld, dt_offset,
                                  Adagrad{r.lr, r.eps, (float* const*)r.state}, sa, pa, [&](const SinglesArgs& s1) {
                                      return launch_adagrad_apply(ctx, ix, tabs, aligned16, T_, D, tdtype, 1, N, dt,
                                                                  DLRM_F32, dt_ld, dt_offset, r, s1, nullptr);
                                  });
}

}  // namespace dlrm
