// mlp_fp8_plan.hpp — the fused MXFP8 MLP inference chain (mlp_fp8.hip): tile height, grid, LDS and the packed layout,
// decided here, once, as a pure function.
//
// Host only, as mlp_plan.hpp: no HIP header, `g++ -std=c++17` compiles it alone.  dlrm_mlp_fp8_plan returns exactly
// this; the launchers read nothing else.  DESIGN.md section 31 restates it.
#pragma once
#include <stdint.h>

#include "../../include/dlrm_hip.h"

namespace dlrm {

constexpr int kFp8MaxLayers = 8;
constexpr int kFp8MaxWidth = 1024;      // the widest padded activation or output a chain may have
constexpr int kFp8Threads = 256;        // four waves: a wave takes the 64-column chunks w, w + 4, ...
constexpr int kFp8RowPad = 16;          // bytes after every LDS code row: rows 16 B off a multiple of 128 B
constexpr int kFp8LdsMax = 160 * 1024;  // gfx950
constexpr int kFp8StaticLds = 2 * kFp8MaxWidth * 4;  // the kernel's own: two layers' fp32 biases
// the tile rule (measured at B = 2048 and 8192 only; 64-row tiles lost at both and are taken
// only when forced)
constexpr int kFp8MT32Batch = 4096;     // batches from here on take 32-row tiles

// Layer l is a_{l+1}[N] = act(W[N][K] a_l[K] + b[N]) with K = sizes[l], N = sizes[l + 1].
struct MlpFp8Plan {
    int layers = 0;
    int MT = 0;             // batch rows per workgroup: 16 or 32 by the rule, 64 when forced
    int grid = 0;           // ceil(batch / MT) workgroups of kFp8Threads
    int wmax = 0;           // the widest LDS-resident activation: max over layers of Kp
    int64_t lds_bytes = 0;  // two buffers of MT x (wmax + kFp8RowPad) codes and MT x wmax / 32 scale bytes
    int K[kFp8MaxLayers], N[kFp8MaxLayers];
    int Kp[kFp8MaxLayers];  // ceil128(K): k-steps of 128
    int Np[kFp8MaxLayers];  // ceil16(N): n-blocks of 16
    // the packed buffer (bytes, every offset a multiple of 64): layer l's e4m3 codes [Np/16][Kp/128][64 lanes][32 B] at
    // w_off[l], their E8M0 scale bytes [Np/16][Kp/128][64 lanes] at s_off[l], its fp32 bias [Np] at b_off[l]
    int64_t w_off[kFp8MaxLayers], s_off[kFp8MaxLayers], b_off[kFp8MaxLayers];
    int64_t packed_bytes = 0;
};

inline int mlp_fp8_ceil(int v, int m) { return (v + m - 1) / m * m; }

// sizes: layers + 1 widths.  batch >= 0 (0: an empty grid).  force_mt: 0, or the tile height to take instead of the
// rule's (the comparison knob DLRM_MLP_FP8_MT).  The dtypes are of x and out: fp32 or bf16.
inline int plan_mlp_fp8(int layers, const int* sizes, int batch, int x_dtype, int out_dtype, int force_mt, MlpFp8Plan* p) {
    if (!p || layers <= 0 || !sizes || batch < 0) return DLRM_E_ARG;
    if ((x_dtype != DLRM_F32 && x_dtype != DLRM_BF16) || (out_dtype != DLRM_F32 && out_dtype != DLRM_BF16))
        return DLRM_E_ARG;
    if (force_mt != 0 && force_mt != 16 && force_mt != 32 && force_mt != 64) return DLRM_E_ARG;
    if (layers > kFp8MaxLayers) return DLRM_E_UNSUPPORTED;
    for (int l = 0; l <= layers; ++l) {
        if (sizes[l] <= 0) return DLRM_E_ARG;
        if (mlp_fp8_ceil(sizes[l], 16) > kFp8MaxWidth) return DLRM_E_UNSUPPORTED;
    }
    MlpFp8Plan q;
    q.layers = layers;
    int64_t off = 0;
    for (int l = 0; l < layers; ++l) {
        q.K[l] = sizes[l];
        q.N[l] = sizes[l + 1];
        q.Kp[l] = mlp_fp8_ceil(sizes[l], 128);
        q.Np[l] = mlp_fp8_ceil(sizes[l + 1], 16);
        if (q.Kp[l] > q.wmax) q.wmax = q.Kp[l];
        q.w_off[l] = off;
        off += (int64_t)q.Np[l] * q.Kp[l];  // (a multiple of 2 KB)
        q.s_off[l] = off;
        off += (int64_t)q.Np[l] * q.Kp[l] / 32;  // (a multiple of 64 B)
    }
    for (int l = 0; l < layers; ++l) {
        q.b_off[l] = off;
        off += (int64_t)q.Np[l] * 4;  // (a multiple of 64 B)
    }
    for (int l = layers; l < kFp8MaxLayers; ++l)
        q.K[l] = q.N[l] = q.Kp[l] = q.Np[l] = 0, q.w_off[l] = q.s_off[l] = q.b_off[l] = 0;
    q.packed_bytes = off;
    q.MT = force_mt ? force_mt : (batch >= kFp8MT32Batch ? 32 : 16);
    q.grid = (batch + q.MT - 1) / q.MT;
    q.lds_bytes = 2 * (int64_t)q.MT * (q.wmax + kFp8RowPad + q.wmax / 32);
    if (q.lds_bytes > kFp8LdsMax - kFp8StaticLds) return DLRM_E_UNSUPPORTED;  // (not reached: kFp8MaxWidth gives 134 KB)
    *p = q;
    return DLRM_OK;
}

}  // namespace dlrm
