// mlp_fp8.hpp — the fused MXFP8 MLP inference chain: mlp_fp8.hip's launchers (called by abi.cpp).
#pragma once
#include "common.hpp"
#include "mlp_fp8_plan.hpp"

namespace dlrm {

// Raises the chain kernels' dynamic-LDS limit to kFp8LdsMax - kFp8StaticLds: off the launch path (a create's job).
int mlp_fp8_prepare(dlrm_ctx* ctx);
// One launch for every layer: W[l] fp32 [N][K] with leading dimension w_ld[l], b[l] fp32 [N] -> packed
// (mlp_fp8_plan.hpp), quantised to MXFP8 on the device.
int launch_mlp_fp8_pack(dlrm_ctx* ctx, const MlpFp8Plan& p, void* packed, const float* const* W, const int64_t* w_ld,
                        const float* const* b);
// One launch for the whole chain; p is the plan of this batch and these dtypes.
int launch_mlp_fp8_chain(dlrm_ctx* ctx, const MlpFp8Plan& p, const void* packed, int batch, const void* x, int x_dtype,
                         int64_t x_ld, void* out, int out_dtype, int64_t out_ld, bool last_relu);

}  // namespace dlrm
