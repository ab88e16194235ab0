// sr_adagrad_step.hip — the apply launch of the training step with the element-wise Adagrad rule and the stochastic
// store on bf16 tables (gfx950) when it carries the next batch's split indexer build
// (dlrm_sr_adagrad_step_bwd_prepare): apply.hpp's StochasticAdagrad rule in MODE 2 / 3 / 5.  Only bf16 tables and the
// step's fp32 dt rows are instantiated.  MODE 0 and 1 stay in sr_adagrad.hip.
//
// The step word is sr_step.hip's: the backward launch and this launch of one training step read the same value, and
// the one-thread advance follows the launch that ran the apply.
#include "apply_kernel.hpp"

namespace dlrm {
extern template ApplyFn launch_rule_apply<StochasticAdagrad>;
template ApplyFn launch_rule_step_apply<StochasticAdagrad>;
}  // namespace dlrm
