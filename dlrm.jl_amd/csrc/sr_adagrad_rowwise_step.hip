// sr_adagrad_rowwise_step.hip — the apply launch of the training step with the row-wise Adagrad rule and the
// stochastic store on bf16 tables (gfx950) when it carries the next batch's split indexer build
// (dlrm_sr_adagrad_step_bwd_prepare): apply.hpp's StochasticRowwiseAdagrad rule in MODE 2 / 3 / 5.  Only bf16 tables
// and the step's fp32 dt rows are instantiated.  MODE 0 and 1 stay in sr_adagrad_rowwise.hip; the step word is read
// and advanced as in sr_adagrad_step.hip.
#include "apply_kernel.hpp"

namespace dlrm {
extern template ApplyFn launch_rule_apply<StochasticRowwiseAdagrad>;
template ApplyFn launch_rule_step_apply<StochasticRowwiseAdagrad>;
}  // namespace dlrm
