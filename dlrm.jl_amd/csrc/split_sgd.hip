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

// (r.state: the device array of per-table uint16 [nrows][D] low-half pointers; tdtype: bf16, the caller checked)
int launch_split_sgd_apply(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, int T_, int D, int,
                           int L, int64_t N, const void* grad, int gdtype, int64_t grad_ld, int64_t grad_offset,
                           const BoundRule& r, const SinglesArgs& sa, const PrepArgs*) {
    return launch_apply_rule(ctx, ix, tabs, aligned16, T_, D, DLRM_BF16, L, N, grad, gdtype, grad_ld, grad_offset,
                             SplitDescent{r.lr, (uint16_t* const*)r.state}, sa, nullptr);
}

}  // namespace dlrm
