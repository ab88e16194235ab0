// mlp_plan.hpp — the fused bf16 MLP inference chain (mlp_bf16.hip): tile height, grid, LDS and the packed layout,
// decided here, once, as a pure function.
//
// Host only, as q8_plan.hpp / interact_plan.hpp: no HIP header, `g++ -std=c++17` compiles it alone.  dlrm_mlp_bf16_plan
// returns exactly this; the handle (abi.cpp) keeps one per batch it is asked for and the launchers read nothing else.
// DESIGN.md section 26 restates it.
#pragma once
#include <stdint.h>

#include "../../include/dlrm_hip.h"

namespace dlrm {

constexpr int kMlpMaxLayers = 8;
constexpr int kMlpMaxWidth = 1024;     // the widest padded activation or output a chain may have
constexpr int kMlpThreads = 256;       // four waves: a wave takes the 64-column chunks w, w + 4, ...
constexpr int kMlpRowPad = 8;          // bf16 elements after every LDS row: rows 16 B off a multiple of 128 B
constexpr int kMlpLdsMax = 160 * 1024; // gfx950
constexpr int kMlpStaticLds = 2 * kMlpMaxWidth * 4;  // the kernel's own: two layers' fp32 biases, beside the dynamic LDS
constexpr int kMlpMT32Batch = 4096;    // batches from here on take 32-row tiles (measured)

// Layer l is a_{l+1}[N] = act(W[N][K] a_l[K] + b[N]) with K = sizes[l], N = sizes[l + 1].
struct MlpPlan {
    int layers = 0;
    int MT = 0;             // batch rows per workgroup: 16 or 32
    int grid = 0;           // ceil(batch / MT) workgroups of kMlpThreads
    int wmax = 0;           // the widest LDS-resident activation: max over layers of Kp
    int64_t lds_bytes = 0;  // two buffers of MT x (wmax + kMlpRowPad) bf16
    int K[kMlpMaxLayers], N[kMlpMaxLayers];
    int Kp[kMlpMaxLayers];  // ceil32(K): k-steps of 32
    int Np[kMlpMaxLayers];  // ceil16(N): n-blocks of 16
    // the packed buffer: layer l's weights [Np/16][Kp/32][64 lanes][8 bf16] at w_off[l], its fp32 bias [Np] at b_off[l]
    // (bytes, every one a multiple of 64), packed_bytes in all
    int64_t w_off[kMlpMaxLayers], b_off[kMlpMaxLayers];
    int64_t packed_bytes = 0;
};

inline int mlp_ceil(int v, int m) { return (v + m - 1) / m * m; }

// sizes: layers + 1 widths.  batch >= 0 (0: an empty grid).  force_mt: 0, or the tile height to take instead of the
// rule's (the comparison knob DLRM_MLP_MT).  The dtypes are of x and out: fp32 or bf16, checked here so that the
// launcher's switch has no other case.
inline int plan_mlp(int layers, const int* sizes, int batch, int x_dtype, int out_dtype, int force_mt, MlpPlan* p) {
    if (!p || layers <= 0 || !sizes || batch < 0) return DLRM_E_ARG;
    if ((x_dtype != DLRM_F32 && x_dtype != DLRM_BF16) || (out_dtype != DLRM_F32 && out_dtype != DLRM_BF16))
        return DLRM_E_ARG;
    if (force_mt != 0 && force_mt != 16 && force_mt != 32) return DLRM_E_ARG;
    if (layers > kMlpMaxLayers) return DLRM_E_UNSUPPORTED;
    for (int l = 0; l <= layers; ++l) {
        if (sizes[l] <= 0) return DLRM_E_ARG;
        if (mlp_ceil(sizes[l], 16) > kMlpMaxWidth) return DLRM_E_UNSUPPORTED;
    }
    MlpPlan q;
    q.layers = layers;
    int64_t off = 0;
    for (int l = 0; l < layers; ++l) {
        q.K[l] = sizes[l];
        q.N[l] = sizes[l + 1];
        q.Kp[l] = mlp_ceil(sizes[l], 32);
        q.Np[l] = mlp_ceil(sizes[l + 1], 16);
        if (q.Kp[l] > q.wmax) q.wmax = q.Kp[l];
        q.w_off[l] = off;
        off += (int64_t)q.Np[l] * q.Kp[l] * 2;  // (a multiple of 1 KB)
    }
    for (int l = 0; l < layers; ++l) {
        q.b_off[l] = off;
        off += (int64_t)q.Np[l] * 4;  // (a multiple of 64 B)
    }
    for (int l = layers; l < kMlpMaxLayers; ++l) q.K[l] = q.N[l] = q.Kp[l] = q.Np[l] = 0, q.w_off[l] = q.b_off[l] = 0;
    q.packed_bytes = off;
    q.MT = force_mt ? force_mt : (batch >= kMlpMT32Batch ? 32 : 16);
    q.grid = (batch + q.MT - 1) / q.MT;
    q.lds_bytes = 2 * (int64_t)q.MT * (q.wmax + kMlpRowPad) * 2;
    if (q.lds_bytes > kMlpLdsMax - kMlpStaticLds) return DLRM_E_UNSUPPORTED;  // (not reached: kMlpMaxWidth gives 129 KB)
    *p = q;
    return DLRM_OK;
}

}  // namespace dlrm
