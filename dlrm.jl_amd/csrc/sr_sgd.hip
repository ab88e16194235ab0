// sr_sgd.hip — update!(Descent(lr), ...) on bf16 tables with a stochastically rounded store (gfx950): an
// unbiased step that costs no memory beside the table.
//
// The apply launch of update.hip (apply_kernel.hpp: one write per touched row, the row's whole gradient sum G
// in hand at the write) with apply.hpp's StochasticDescent rule at its write sites:
//   W' = fmaf(-lr, G, w);  w = sr_bf16(W', R),  R = 16 Philox4x32-10 bits of (seed, step, table, row, column)
// No state stream: the row is loaded where Descent loads it and written once.  Only bf16 tables (TT =
// uint16_t) are instantiated, MODE 0 and 1.  The step is a device word of the optimizer handle: every launch of
// a call reads it, and a one-thread launch after the call's last adds one, in stream order (so a captured
// update advances it on every replay and nothing synchronises).  The fused training step with the rule
// (dlrm_sr_step_bwd) reads the same word in its backward and its apply (sr_step.hip) and advances it the same way.
#include "apply_kernel.hpp"

namespace dlrm {

__global__ void sr_step_advance_kernel(uint64_t* step) { *step += 1; }
__global__ void sr_step_set_kernel(uint64_t* step, uint64_t value) { *step = value; }

// (tdtype: bf16, the caller checked)
int launch_sr_sgd_apply(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, int T_, int D, int, int L,
                        int64_t N, const void* grad, int gdtype, int64_t grad_ld, int64_t grad_offset,
                        const BoundRule& r, const SinglesArgs& sa, const PrepArgs*) {
    if (T_ == 0 || N == 0) return DLRM_OK;  // (nothing launched: the step stays)
    const int rc = launch_apply_rule(ctx, ix, tabs, aligned16, T_, D, DLRM_BF16, L, N, grad, gdtype, grad_ld, grad_offset,
                                     StochasticDescent{r.lr, (uint32_t)r.seed, (uint32_t)(r.seed >> 32), r.step, 0u, 0u},
                                     sa, nullptr);
    if (rc) return rc;
    return launch_sr_step_advance(ctx, r.step);
}

// after a call's last launch that reads the word: every workgroup of it has read the word when this one starts
int launch_sr_step_advance(dlrm_ctx* ctx, uint64_t* step) {
    hipLaunchKernelGGL(sr_step_advance_kernel, dim3(1), dim3(1), 0, ctx_stream(ctx), step);
    return ctx_hip(ctx, hipGetLastError(), "sr_step_advance launch");
}

int launch_sr_step_set(dlrm_ctx* ctx, uint64_t* step, uint64_t value) {
    hipLaunchKernelGGL(sr_step_set_kernel, dim3(1), dim3(1), 0, ctx_stream(ctx), step, value);
    return ctx_hip(ctx, hipGetLastError(), "sr_step_set launch");
}

}  // namespace dlrm
