// split_step.hip — the apply launch of the training step on split-bf16 tables (gfx950) when it carries the next
// batch's split indexer build (dlrm_split_step_bwd_prepare): apply.hpp's SplitDescent rule in MODE 2 / 3 / 5.
// Only bf16 tables and the step's fp32 dt rows are instantiated.  MODE 0 and 1 stay in split_sgd.hip.
#include "apply_kernel.hpp"

namespace dlrm {
extern template ApplyFn launch_rule_apply<SplitDescent>;
template ApplyFn launch_rule_step_apply<SplitDescent>;
}  // namespace dlrm
