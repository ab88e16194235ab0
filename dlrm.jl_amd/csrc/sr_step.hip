// sr_step.hip — the apply launch of the training step with the stochastic rule on bf16 tables (gfx950) when it
// carries the next batch's split indexer build (dlrm_sr_step_bwd_prepare), and the advance of the step word that
// ends every such step.
//
// apply.hpp's StochasticDescent rule in MODE 2 / 3 / 5 (the build's workgroups first, then chunks and hot slices; no
// once-hit items: the step backward stepped those rows).  Only bf16 tables and the step's fp32 dt rows are
// instantiated.  MODE 0 and 1 stay in sr_sgd.hip; the two units compile beside update.hip.
//
// The step word: the backward launch and this launch of one training step read the same value (every workgroup
// once, StochasticDescent::load_step); the one-thread advance follows the launch that ran the apply, in stream
// order.
#include "apply_kernel.hpp"

namespace dlrm {
extern template ApplyFn launch_rule_apply<StochasticDescent>;
template ApplyFn launch_rule_step_apply<StochasticDescent>;
}  // namespace dlrm
