// mlp_train_plan.hpp — bf16 MLP training (mlp_train.hip): padded sizes, buffer layout, tiles, grids and the wgrad
// slab rule, decided here, once, as a pure function.
//
// Host only, as mlp_plan.hpp: no HIP header, `g++ -std=c++17` compiles it alone.  dlrm_mlp_train_plan returns
// exactly this; the handle (abi.cpp) keeps the layout of its max_batch and the launchers read nothing else.
// DESIGN.md section 28 restates it.
#pragma once
#include <stdint.h>

#include "../../include/dlrm_hip.h"

namespace dlrm {

constexpr int kMtMaxLayers = 8;
constexpr int kMtMaxWidth = 8192;  // the widest level a chain may have
constexpr int kMtThreads = 256;    // four waves, 2 x 2, a 32 x 32 register tile each
constexpr int kMtTile = 64;        // an output tile is 64 x 64 and a k-step 64: every role
constexpr int kMtRowPad = 8;       // bf16 elements after every LDS row: rows 16 B off a multiple of 128 B
constexpr int kMtCUs = 256;        // the slab rule's target: a wgrad launch has at least this many workgroups ...
constexpr int kMtMaxSlabs = 32;    // ... where the batch allows, and at most this many slabs
enum { kMtFwd = 0, kMtDgrad = 1, kMtWgrad = 2 };

inline int mt_ceil(int v, int m) { return (v + m - 1) / m * m; }
inline int64_t mt_align(int64_t v) { return (v + 255) / 256 * 256; }

// The slabs of a wgrad whose output has `tiles` tiles over a batch of `ksteps` k-steps: the fewest that reach kMtCUs
// workgroups, none empty.  rows: the slab's batch rows.
inline int mt_slabs(int tiles, int ksteps, int* rows) {
    int want = (kMtCUs + tiles - 1) / tiles;
    if (want > kMtMaxSlabs) want = kMtMaxSlabs;
    if (want > ksteps) want = ksteps;
    const int per = (ksteps + want - 1) / want;
    if (rows) *rows = per * kMtTile;
    return (ksteps + per - 1) / per;
}

// sizes: layers + 1 widths; batch >= 1.
inline int plan_mlp_train(int layers, const int* sizes, int batch, dlrm_mlp_train_layout* p) {
    if (!p || layers <= 0 || !sizes || batch <= 0) return DLRM_E_ARG;
    if (layers > kMtMaxLayers) return DLRM_E_UNSUPPORTED;
    for (int l = 0; l <= layers; ++l) {
        if (sizes[l] <= 0) return DLRM_E_ARG;
        if (sizes[l] > kMtMaxWidth) return DLRM_E_UNSUPPORTED;
    }
    dlrm_mlp_train_layout q = {};
    q.layers = layers;
    q.batch = batch;
    q.ldt = mt_ceil(batch, kMtTile);
    for (int r = 0; r < 3; ++r) q.tile[r][0] = q.tile[r][1] = q.tile[r][2] = kMtTile;
    for (int i = 0; i <= layers; ++i) q.ld[i] = mt_ceil(sizes[i], kMtTile);
    const int mtiles = q.ldt / kMtTile;
    int64_t w = 0, a = 0, g = 0, pp = 0;
    for (int l = 0; l < layers; ++l) {
        const int K = sizes[l], N = sizes[l + 1];
        const int kt = q.ld[l] / kMtTile, nt = q.ld[l + 1] / kMtTile;
        q.slabs[l] = mt_slabs(nt * kt, mtiles, &q.slab_rows[l]);
        const int grid[3][3] = {{nt, mtiles, 1}, {kt, mtiles, 1}, {nt, kt, q.slabs[l]}};
        for (int r = 0; r < 3; ++r)
            for (int d = 0; d < 3; ++d) q.grid[l][r][d] = grid[r][d];
        q.w_off[l] = w;
        w += mt_align((int64_t)N * q.ld[l] * 2);
        q.wt_off[l] = w;
        w += mt_align((int64_t)K * q.ld[l + 1] * 2);
        // level l (the layer's input) and level l + 1 (its output's gradient)
        q.a_off[l] = a;
        a += mt_align((int64_t)batch * q.ld[l] * 2);
        q.at_off[l] = a;
        a += mt_align((int64_t)K * q.ldt * 2);
        q.g_off[l] = g;
        g += mt_align((int64_t)batch * q.ld[l + 1] * 2);
        q.gt_off[l] = g;
        g += mt_align((int64_t)N * q.ldt * 2);
        q.p_off[l] = pp;
        if (q.slabs[l] > 1) pp += mt_align((int64_t)q.slabs[l] * N * K * 4);
        q.pb_off[l] = pp;
        if (q.slabs[l] > 1) pp += mt_align((int64_t)q.slabs[l] * N * 4);
    }
    q.w_bytes = w;
    q.a_bytes = a;
    q.g_bytes = g;
    q.p_bytes = pp > 0 ? pp : 256;
    *p = q;
    return DLRM_OK;
}

}  // namespace dlrm
