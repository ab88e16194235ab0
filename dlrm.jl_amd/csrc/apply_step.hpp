// apply_step.hpp -- the apply launch of the training step with the split rule (dlrm_split_step_bwd[_prepare]), a
// sparse Adagrad rule (dlrm_adagrad_step_bwd[_prepare]), the stochastic rule (dlrm_sr_step_bwd[_prepare]) or a seeded
// Adagrad rule (dlrm_sr_adagrad_step_bwd[_prepare]) when it carries the next batch's split indexer build.
//
// apply_kernel.hpp's launch in MODE 2 / 3 / 5 (the build's workgroups first, then chunks and hot slices; no
// once-hit items: the step backward stepped those rows) with the rule at its write sites.  Only what the step
// needs is instantiated: fp32 (a rule with kF32Tables) and bf16 tables, the step's fp32 dt rows.  MODE 0 and 1 stay
// in split_sgd.hip, adagrad.hip, adagrad_rowwise.hip and sr_sgd.hip; split_step.hip, adagrad_step.hip,
// adagrad_rowwise_step.hip, sr_step.hip, sr_adagrad_step.hip and sr_adagrad_rowwise_step.hip include this, one rule
// each, and compile beside update.hip.
#pragma once
#include "apply_kernel.hpp"

namespace dlrm {

// plain(sa): the rule's MODE 0 / 1 launch (its own unit's).  (A rule without kF32Tables: the caller checked that the
// tables are bf16, as by_dtypes' callers do.)
template <typename R, typename Plain>
static int launch_step_apply_rule(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool aligned16, int T_, int D,
                                  int tdtype, int64_t N, const float* dt, int64_t dt_ld, int64_t dt_offset,
                                  const R& rule, const SinglesArgs& sa, const PrepArgs* pa, Plain&& plain) {
    // launch_apply_rule's conditions for the vector kernels (fp32 gradient rows)
    const int TV = T_ << ix.vshift;  // virtual tables (row-parity halves) of a forward-launch build
    const int tesz = tdtype == DLRM_F32 ? 4 : 2;
    const bool vec = aligned16 && (uintptr_t)dt % 16 == 0 && (dt_ld * 4) % 16 == 0 && (dt_offset * 4) % 16 == 0 &&
                     D % 4 == 0 && (D * tesz) % 16 == 0 && (int64_t)TV * (N + 1) < (1ll << 31);
    if (pa && !sa.single && vec && T_ > 0 && N > 0) {
        hipStream_t s = ctx_stream(ctx);
        const unsigned* err = ctx_error_word(ctx);
        bool done = true;
        switch (D / 4) {  // 16-B vectors per fp32 gradient row
#define DLRM_CASE(V)                                                                                                   \
    case V:                                                                                                            \
        if (tdtype == DLRM_F32) {                                                                                      \
            if constexpr (R::kF32Tables)                                                                               \
                launch_apply_build_vec<float, float, V, R, 2>(s, ix, tabs, TV, 1, dt, dt_ld, dt_offset, rule, N, err, sa, \
                                                              *pa);                                                    \
        } else                                                                                                         \
            launch_apply_build_vec<uint16_t, float, V, R, 2>(s, ix, tabs, TV, 1, dt, dt_ld, dt_offset, rule, N, err, sa, \
                                                             *pa);                                                     \
        break;
            DLRM_CASE(2) DLRM_CASE(4) DLRM_CASE(8) DLRM_CASE(16) DLRM_CASE(32) DLRM_CASE(64) DLRM_CASE(128)
#undef DLRM_CASE
            default: done = false;
        }
        if (done) return ctx_hip(ctx, hipGetLastError(), "step apply(+build) launch");
    }
    // once-hit items in this launch, or no vector kernel for the shape: the rule's own launches, then the build's
    const int rc = plain(sa);
    if (rc == DLRM_OK && pa) {
        launch_step_index(ctx_stream(ctx), *pa);
        return ctx_hip(ctx, hipGetLastError(), "step_index launch");
    }
    return rc;
}

}  // namespace dlrm
