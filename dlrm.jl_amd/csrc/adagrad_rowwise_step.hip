// adagrad_rowwise_step.hip — the apply launch of the training step with the row-wise Adagrad rule (gfx950) when
// it carries the next batch's split indexer build (dlrm_adagrad_step_bwd_prepare): apply.hpp's RowwiseAdagrad rule
// in MODE 2 / 3 / 5.  MODE 0 and 1 stay in adagrad_rowwise.hip.
#include "apply_kernel.hpp"

namespace dlrm {
extern template ApplyFn launch_rule_apply<RowwiseAdagrad>;
template ApplyFn launch_rule_step_apply<RowwiseAdagrad>;
}  // namespace dlrm
