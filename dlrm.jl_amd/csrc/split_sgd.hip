// split_sgd.hip — update!(Descent(lr), ...) on split-bf16 tables (gfx950): an exact fp32 step on rows
// whose high 16 bits live in the bf16 table and whose low 16 bits live in a second uint16 array.
//
// The apply launch of update.hip (apply_kernel.hpp: one write per touched row, the row's whole
// gradient sum G in hand at the write) with apply.hpp's SplitDescent rule at its write sites:
//   W  = bits(hi << 16 | lo);  W' = fmaf(-lr, G, W);  hi' = bits(W') >> 16;  lo' = bits(W') & 0xffff
// Both halves of a row are loaded where Descent loads its table row and written once, with plain
// vector stores.  Only bf16 tables (TT = uint16_t) are instantiated.
#include "apply_kernel.hpp"

namespace dlrm {
template ApplyFn launch_rule_apply<SplitDescent>;
}  // namespace dlrm
