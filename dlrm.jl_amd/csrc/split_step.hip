// split_step.hip — the apply launch of the training step on split-bf16 tables (gfx950) when it carries
// the next batch's split indexer build (dlrm_split_step_bwd_prepare).
//
// apply_kernel.hpp's launch in MODE 2 / 3 / 5 (the build's workgroups first, then chunks and hot slices; no
// once-hit items: the split backward stepped those rows) with apply.hpp's SplitDescent rule at its write
// sites.  Only what the step needs is instantiated: bf16 tables and the step's fp32 dt rows.  MODE 0 and 1
// stay in split_sgd.hip; the two units compile beside update.hip.
#include "apply_kernel.hpp"

namespace dlrm {

int launch_split_step_apply(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, uint16_t* const* lo,
                            int T_, int D, int64_t N, const float* dt, int64_t dt_ld, int64_t dt_offset, float lr,
                            const SinglesArgs& sa, const PrepArgs* pa) {
    // launch_apply_rule's conditions for the vector kernels (bf16 tables, fp32 gradient rows)
    const int TV = T_ << ix.vshift;  // virtual tables (row-parity halves) of a forward-launch build
    const bool vec = aligned16 && (uintptr_t)dt % 16 == 0 && (dt_ld * 4) % 16 == 0 && (dt_offset * 4) % 16 == 0 &&
                     (D * 2) % 16 == 0 && (int64_t)TV * (N + 1) < (1ll << 31);
    if (pa && !sa.single && vec && T_ > 0 && N > 0) {
        hipStream_t s = ctx_stream(ctx);
        const unsigned* err = ctx_error_word(ctx);
        const SplitDescent rule{lr, lo};
        bool done = true;
        switch (D / 4) {  // 16-B vectors per fp32 gradient row
#define DLRM_CASE(V)                                                                                                     \
    case V:                                                                                                              \
        launch_apply_build_vec<uint16_t, float, V, SplitDescent, 2>(s, ix, tabs, TV, 1, dt, dt_ld, dt_offset, rule, N, err, \
                                                                    sa, *pa);                                           \
        break;
            DLRM_CASE(2) DLRM_CASE(4) DLRM_CASE(8) DLRM_CASE(16) DLRM_CASE(32) DLRM_CASE(64) DLRM_CASE(128)
#undef DLRM_CASE
            default: done = false;
        }
        if (done) return ctx_hip(ctx, hipGetLastError(), "split apply(+build) launch");
    }
    // once-hit items in this launch, or no vector kernel for the shape: the rule's own launches, then the build's
    const int rc = launch_split_sgd_apply(ctx, ix, tabs, aligned16, lo, T_, D, 1, N, dt, DLRM_F32, dt_ld, dt_offset, lr, sa);
    if (rc == DLRM_OK && pa) {
        launch_step_index(ctx_stream(ctx), *pa);
        return ctx_hip(ctx, hipGetLastError(), "step_index launch");
    }
    return rc;
}

}  // namespace dlrm
