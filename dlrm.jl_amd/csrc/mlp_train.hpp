// mlp_train.hpp — bf16 MLP training: mlp_train.hip's launchers (called by abi.cpp).
#pragma once
#include "common.hpp"
#include "mlp_train_plan.hpp"

namespace dlrm {

// L is the layout of the handle's max_batch (the buffers' offsets); batch <= L.batch is this call's.
// One launch: every layer's W16 and W16T from the fp32 masters.
int launch_mlp_train_refresh(dlrm_ctx* ctx, const dlrm_mlp_train_layout& L, const int* sizes, const float* const* W,
                             const int64_t* w_ld, void* w16);
// One conversion launch (level 0) and one GEMM launch per layer.
int launch_mlp_train_forward(dlrm_ctx* ctx, const dlrm_mlp_train_layout& L, const int* sizes, int batch, const void* x,
                             int x_dtype, int64_t x_ld, const float* const* b, const void* w16, void* acts, void* out,
                             int out_dtype, int64_t out_ld, bool last_relu);
// One conversion launch (g_n), a wgrad and a dgrad launch per layer (no dgrad of layer 1 without dx), and one launch
// that sums the slab partials where a layer has slabs.
int launch_mlp_train_backward(dlrm_ctx* ctx, const dlrm_mlp_train_layout& L, const int* sizes, int batch, const void* dy,
                              int dy_dtype, int64_t dy_ld, const void* out, int out_dtype, int64_t out_ld,
                              const void* w16, const void* acts, void* grads, void* part, float* const* gW,
                              const int64_t* gw_ld, float* const* gb, bool write_last_gb, void* dx, int dx_dtype,
                              int64_t dx_ld);

}  // namespace dlrm
