// mlp_train.hip — mixed-precision training of a Dense chain on gfx950 MFMA: forward, dgrad and wgrad.
//
// fp32 master weights, bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 accumulation.  One tiled GEMM core,
//     C[i][j] = sum_k A[i][k] B[j][k]        (both operands row-major with the contraction index contiguous)
// serves the three roles; what differs is which tensors are A and B and the epilogue:
//     forward   A = W16_l   [N][Kp]    B = a_{l-1} [B][Kp]    i = n, j = m, k = k    bias, relu, bf16 store(s)
//     dgrad     A = W16T_l  [K][Np]    B = g_l     [B][Np]    i = k, j = m, k = n    relu mask, bf16 store(s)
//     wgrad     A = gT_l    [N][Bp]    B = aT_{l-1}[K][Bp]    i = n, j = k, k = m    fp32 gW (+ gb), slabs
// Dgrad and wgrad contract over an index that is not contiguous in the row-major tensors, so every bf16 tensor is
// kept in both forms, each written by the kernel that produces it: W16 / W16T by the refresh launch, a / aT by the
// forward's epilogue, g / gT by the dgrad's epilogue (level 0 and g_n by the conversion launch).  DESIGN.md section
// 28 says why this and not transposing LDS reads.
//
// Core: a workgroup of four waves (2 x 2) owns a 64 x 64 output tile and walks the contraction in k-steps of 64.
// Both operands are staged through LDS, double-buffered: the 16-B global loads of step s + 1 are issued before the
// MFMAs of step s and written to the other buffer after them, one barrier per step.  LDS rows are 64 + 8 bf16, so a
// wave's 16-B operand reads (lane (c, q): row c, k = 8q .. 8q + 7 of a 32-wide half) are conflict-free.  A wave holds
// 2 x 2 accumulators of 16 x 16, so each operand read feeds two MFMAs.  A is the MFMA's first operand: lane (c, q)
// ends with C[i = 4q .. 4q + 3][j = c], four consecutive i of one j -- which for the forward and the dgrad is four
// consecutive features of one sample (one packed 8-B store, one 8-B mask load) and for the wgrad makes the 16 lanes
// of a quad write 16 consecutive k of one gW row.
// Rows past an operand's last are clamped on load and their results dropped; the contraction needs no tail: every
// leading dimension is a multiple of 64 with zero padding (mlp_train_plan.hpp).
// gb rides in the wgrad: workgroups of the first k-tile issue one more MFMA per A read against an operand of ones,
// which gives the column sums of g_l in the same fp32 accumulation.
// No atomics: a wgrad slab writes its partial tile to its own place and mlp_train_reduce_kernel sums the slabs in
// slab order.
#include "mlp_train.hpp"

namespace dlrm {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// two fp32 -> two bf16 in one word, ties to even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t mt_pack(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){lo, hi}, bf16x2_t));
}
__device__ __forceinline__ uint16_t mt_bf16(float v) { return (uint16_t)(mt_pack(v, 0.0f) & 0xffffu); }
// a stored bf16 activation is > 0: the sign clear and the magnitude not zero
__device__ __forceinline__ bool mt_pos(uint32_t h) { return (h & 0x8000u) == 0u && (h & 0x7fffu) != 0u; }

// ------------------------------------------------------------------------------------------------------ refresh
struct MtRefreshArgs {
    const float* W[kMtMaxLayers];
    int64_t ldw[kMtMaxLayers];
    uint16_t* w[kMtMaxLayers];   // W16  [N][Kp]
    uint16_t* wt[kMtMaxLayers];  // W16T [K][Np]
    int N[kMtMaxLayers], K[kMtMaxLayers], Np[kMtMaxLayers], Kp[kMtMaxLayers];
    int64_t start[kMtMaxLayers + 1];  // 8-element items before the layer: N Kp / 8 of W16, then K Np / 8 of W16T
    int layers;
};

__global__ __launch_bounds__(256) void mlp_train_refresh_kernel(const MtRefreshArgs a) {
    const int64_t total = a.start[a.layers];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int l = 0;
        while (l + 1 < a.layers && i >= a.start[l + 1]) ++l;
        const int64_t j = i - a.start[l];
        const int N = a.N[l], K = a.K[l], Np = a.Np[l], Kp = a.Kp[l];
        const int64_t nw = (int64_t)N * (Kp >> 3);
        const float* W = a.W[l];
        const int64_t ldw = a.ldw[l];
        float f[8];
        uint16_t* dst;
        if (j < nw) {
            const int n = (int)(j / (Kp >> 3)), k0 = (int)(j - (int64_t)n * (Kp >> 3)) * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = k0 + e < K ? ldg<float>(W + (int64_t)n * ldw + k0 + e) : 0.0f;
            dst = a.w[l] + (int64_t)n * Kp + k0;
        } else {
            const int64_t jt = j - nw;
            const int k = (int)(jt / (Np >> 3)), n0 = (int)(jt - (int64_t)k * (Np >> 3)) * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = n0 + e < N ? ldg<float>(W + (int64_t)(n0 + e) * ldw + k) : 0.0f;
            dst = a.wt[l] + (int64_t)k * Np + n0;
        }
        stg<u32x4_t>(dst, u32x4_t{mt_pack(f[0], f[1]), mt_pack(f[2], f[3]), mt_pack(f[4], f[5]), mt_pack(f[6], f[7])});
    }
}

// --------------------------------------------------------------------------------------------------- conversion
// src [B][C] (fp32 or bf16) -> dst [B][Cp] and dstT [C][ldt], bf16; with `mask` only where mask[m][c] > 0.
// Columns C .. Cp of dst and B .. Bp of dstT are written as zero.
__global__ __launch_bounds__(256) void mlp_train_convert_kernel(const void* src, int src_bf16, int64_t ld_src,
                                                                const void* mask, int mask_bf16, int64_t ld_mask,
                                                                uint16_t* dst, int64_t ld_dst, uint16_t* dstT, int64_t ldt,
                                                                int B, int Bp, int C, int Cp) {
    const int64_t total = (int64_t)Bp * Cp;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i / Bp), m = (int)(i - (int64_t)c * Bp);
        float v = 0.0f;
        if (m < B && c < C) {
            v = src_bf16 ? bf16_to_f32(ldg<uint16_t>((const uint16_t*)src + (int64_t)m * ld_src + c))
                         : ldg<float>((const float*)src + (int64_t)m * ld_src + c);
            if (mask) {
                const float y = mask_bf16 ? bf16_to_f32(ldg<uint16_t>((const uint16_t*)mask + (int64_t)m * ld_mask + c))
                                          : ldg<float>((const float*)mask + (int64_t)m * ld_mask + c);
                if (!(y > 0.0f)) v = 0.0f;
            }
        }
        const uint16_t h = mt_bf16(v);
        if (m < B) stg<uint16_t>(dst + (int64_t)m * ld_dst + c, h);
        if (c < C) stg<uint16_t>(dstT + (int64_t)c * ldt + m, h);
    }
}

// --------------------------------------------------------------------------------------------------------- GEMM
struct MtGemmArgs {
    const uint16_t* A;  // [rowsA][lda]: the output's i
    const uint16_t* B;  // [rowsB][ldb]: the output's j
    int64_t lda, ldb;
    int rowsA, rowsB;
    int ksteps, per_slab;  // k-steps of 64 in all and per blockIdx.z
    // forward and dgrad: i is a feature (rowsA of them), j a sample (rowsB = the batch)
    const float* bias;     // forward: fp32 [rowsA]
    int relu;              // forward
    const uint16_t* mask;  // dgrad: the saved activation [batch][ld_mask], or null (layer 1)
    int64_t ld_mask;
    uint16_t* out;         // hidden: bf16 [batch][ld_out] ...
    uint16_t* outT;        // ... and [rowsA][ld_outT]; batch_pad columns are written
    int64_t ld_out, ld_outT;
    void* fin;             // not null: the chain's end -- the only store, in the caller's dtype
    int64_t ld_fin;
    int fin_bf16;
    // wgrad: i = n (rowsA), j = k (rowsB)
    float* gW;             // [rowsA][ld_gw]
    float* gb;             // [rowsA], or null: not written
    int64_t ld_gw;
    float* part;           // slabs > 1: [slabs][rowsA][rowsB] and ...
    float* partb;          // ... [slabs][rowsA] instead
    int slabs;
};

template <int ROLE>
__global__ __launch_bounds__(kMtThreads) void mlp_train_gemm_kernel(const MtGemmArgs a) {
    constexpr int LD = kMtTile + kMtRowPad;
    __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][kMtTile * LD];  // [buffer][operand]
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), wi = w >> 1, wj = w & 1;
    const int i0 = blockIdx.x * kMtTile, j0 = blockIdx.y * kMtTile;
    const int s_begin = blockIdx.z * a.per_slab, s_end = min(s_begin + a.per_slab, a.ksteps);
    const bool ones = ROLE == kMtWgrad && blockIdx.y == 0;  // this workgroup also sums g's columns

    // a thread's share of a k-step: rows lr and lr + 32 of both operands, 8 elements at lc
    const int lr = tid >> 3, lc = (tid & 7) * 8;
    const uint16_t* pa[2];
    const uint16_t* pb[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        pa[h] = a.A + (int64_t)min(i0 + lr + 32 * h, a.rowsA - 1) * a.lda + lc;
        pb[h] = a.B + (int64_t)min(j0 + lr + 32 * h, a.rowsB - 1) * a.ldb + lc;
    }
    u32x4_t ra[2], rb[2];
    auto gload = [&](int s) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            ra[h] = ldg<u32x4_t>(pa[h] + (int64_t)s * kMtTile);
            rb[h] = ldg<u32x4_t>(pb[h] + (int64_t)s * kMtTile);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *(u32x4_t*)&lds[buf][0][(lr + 32 * h) * LD + lc] = ra[h];
            *(u32x4_t*)&lds[buf][1][(lr + 32 * h) * LD + lc] = rb[h];
        }
    };

    f32x4 acc[2][2], accb[2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
        accb[bi] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bf16x8_t one8 = __builtin_bit_cast(bf16x8_t, u32x4_t{0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u});

    if (s_begin < s_end) {
        gload(s_begin);
        lstore(0);
    }
    __syncthreads();
    for (int s = s_begin; s < s_end; ++s) {
        const int buf = (s - s_begin) & 1;
        const bool more = s + 1 < s_end;
        if (more) gload(s + 1);  // in flight under this step's MFMAs
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8_t av[2], bv[2];
#pragma unroll
            for (int b2 = 0; b2 < 2; ++b2) {
                av[b2] = *(const bf16x8_t*)&lds[buf][0][(wi * 32 + b2 * 16 + c) * LD + kk * 32 + 8 * q];
                bv[b2] = *(const bf16x8_t*)&lds[buf][1][(wj * 32 + b2 * 16 + c) * LD + kk * 32 + 8 * q];
            }
#pragma unroll
            for (int bi = 0; bi < 2; ++bi) {
#pragma unroll
                for (int bj = 0; bj < 2; ++bj)
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[bi], bv[bj], acc[bi][bj], 0, 0, 0);
                if (ones) accb[bi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[bi], one8, accb[bi], 0, 0, 0);
            }
        }
        if (more) lstore(buf ^ 1);  // (last read in step s - 1, before its barrier)
        __syncthreads();
    }

    // ---- epilogues: lane (c, q) of block (bi, bj) holds i = ib + 4q + r (r = 0 .. 3), j = jb + c
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
        const int ib = i0 + wi * 32 + bi * 16 + 4 * q;
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
            const int j = j0 + wj * 32 + bj * 16 + c;
            f32x4 v = acc[bi][bj];
            if constexpr (ROLE == kMtWgrad) {
                if (j < a.rowsB) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int n = ib + r;
                        if (n >= a.rowsA) continue;
                        if (a.slabs > 1) stg<float>(a.part + ((int64_t)blockIdx.z * a.rowsA + n) * a.rowsB + j, v[r]);
                        else stg<float>(a.gW + (int64_t)n * a.ld_gw + j, v[r]);
                    }
                }
            } else {
                const int batch = a.rowsB;
                const bool live = j < batch;
                if constexpr (ROLE == kMtFwd) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        v[r] += ib + r < a.rowsA ? ldg<float>(a.bias + ib + r) : 0.0f;
                        if (a.relu) v[r] = v[r] < 0.0f ? 0.0f : v[r];
                    }
                } else if (a.mask) {
                    const u32x2_t y = live ? ldg<u32x2_t>(a.mask + (int64_t)j * a.ld_mask + ib) : u32x2_t{0u, 0u};
                    if (!mt_pos(y[0])) v[0] = 0.0f;
                    if (!mt_pos(y[0] >> 16)) v[1] = 0.0f;
                    if (!mt_pos(y[1])) v[2] = 0.0f;
                    if (!mt_pos(y[1] >> 16)) v[3] = 0.0f;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ib + r >= a.rowsA || !live) v[r] = 0.0f;  // padding columns and padding samples are zero
                if (a.fin) {
                    if (live) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (ib + r >= a.rowsA) continue;
                            const int64_t o = (int64_t)j * a.ld_fin + ib + r;
                            if (a.fin_bf16) stg<uint16_t>((uint16_t*)a.fin + o, mt_bf16(v[r]));
                            else stg<float>((float*)a.fin + o, v[r]);
                        }
                    }
                } else {
                    const u32x2_t h = {mt_pack(v[0], v[1]), mt_pack(v[2], v[3])};
                    if (live) stg<u32x2_t>(a.out + (int64_t)j * a.ld_out + ib, h);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (ib + r < a.rowsA)
                            stg<uint16_t>(a.outT + (int64_t)(ib + r) * a.ld_outT + j, (uint16_t)(h[r >> 1] >> (16 * (r & 1))));
                }
            }
        }
        if constexpr (ROLE == kMtWgrad) {
            if (ones && wj == 0 && c == 0 && a.gb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = ib + r;
                    if (n >= a.rowsA) continue;
                    if (a.slabs > 1) stg<float>(a.partb + (int64_t)blockIdx.z * a.rowsA + n, accb[bi][r]);
                    else stg<float>(a.gb + n, accb[bi][r]);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------- reduce
struct MtReduceArgs {
    const float* part[kMtMaxLayers];
    const float* partb[kMtMaxLayers];
    float* gW[kMtMaxLayers];
    float* gb[kMtMaxLayers];  // null: not written
    int64_t ld_gw[kMtMaxLayers];
    int N[kMtMaxLayers], K[kMtMaxLayers], slabs[kMtMaxLayers];
    int64_t start[kMtMaxLayers + 1];  // items before the layer: N K of gW, then N of gb (none without slabs)
    int layers;
};

__global__ __launch_bounds__(256) void mlp_train_reduce_kernel(const MtReduceArgs a) {
    const int64_t total = a.start[a.layers];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int l = 0;
        while (l + 1 < a.layers && i >= a.start[l + 1]) ++l;
        const int64_t j = i - a.start[l];
        const int N = a.N[l], K = a.K[l], S = a.slabs[l];
        const int64_t nk = (int64_t)N * K;
        if (j < nk) {
            float s = ldg<float>(a.part[l] + j);
            for (int z = 1; z < S; ++z) s += ldg<float>(a.part[l] + z * nk + j);  // slab order
            const int n = (int)(j / K);
            stg<float>(a.gW[l] + (int64_t)n * a.ld_gw[l] + (j - (int64_t)n * K), s);
        } else if (a.gb[l]) {
            const int n = (int)(j - nk);
            float s = ldg<float>(a.partb[l] + n);
            for (int z = 1; z < S; ++z) s += ldg<float>(a.partb[l] + (int64_t)z * N + n);
            stg<float>(a.gb[l] + n, s);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- launchers
static unsigned mt_blocks(dlrm_ctx* ctx, int64_t items) {
    const int64_t blocks = (items + 255) / 256, cap = (int64_t)ctx_num_cus(ctx) * 8;
    return (unsigned)(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}
static uint16_t* mt_at(const void* base, int64_t off) { return (uint16_t*)((char*)base + off); }

int launch_mlp_train_refresh(dlrm_ctx* ctx, const dlrm_mlp_train_layout& L, const int* sizes, const float* const* W,
                             const int64_t* w_ld, void* w16) {
    MtRefreshArgs a{};
    a.layers = L.layers;
    for (int l = 0; l < L.layers; ++l) {
        a.W[l] = W[l];
        a.ldw[l] = w_ld[l];
        a.w[l] = mt_at(w16, L.w_off[l]);
        a.wt[l] = mt_at(w16, L.wt_off[l]);
        a.K[l] = sizes[l];
        a.N[l] = sizes[l + 1];
        a.Kp[l] = L.ld[l];
        a.Np[l] = L.ld[l + 1];
        a.start[l + 1] = a.start[l] + (int64_t)a.N[l] * (a.Kp[l] / 8) + (int64_t)a.K[l] * (a.Np[l] / 8);
    }
    hipLaunchKernelGGL(mlp_train_refresh_kernel, dim3(mt_blocks(ctx, a.start[L.layers])), dim3(256), 0, ctx_stream(ctx), a);
    return ctx_hip(ctx, hipGetLastError(), "mlp_train_refresh launch");
}

static int mt_convert(dlrm_ctx* ctx, const void* src, int src_dtype, int64_t ld_src, const void* mask, int mask_dtype,
                      int64_t ld_mask, uint16_t* dst, int64_t ld_dst, uint16_t* dstT, int64_t ldt, int B, int C) {
    const int Bp = mt_ceil(B, kMtTile), Cp = (int)ld_dst;
    hipLaunchKernelGGL(mlp_train_convert_kernel, dim3(mt_blocks(ctx, (int64_t)Bp * Cp)), dim3(256), 0, ctx_stream(ctx), src,
                       (int)(src_dtype == DLRM_BF16), ld_src, mask, (int)(mask_dtype == DLRM_BF16), ld_mask, dst, ld_dst,
                       dstT, ldt, B, Bp, C, Cp);
    return ctx_hip(ctx, hipGetLastError(), "mlp_train_convert launch");
}

template <int ROLE>
static int mt_gemm(dlrm_ctx* ctx, const MtGemmArgs& a, int gz, const char* what) {
    const dim3 grid((a.rowsA + kMtTile - 1) / kMtTile, (a.rowsB + kMtTile - 1) / kMtTile, gz);
    hipLaunchKernelGGL(mlp_train_gemm_kernel<ROLE>, grid, dim3(kMtThreads), 0, ctx_stream(ctx), a);
    return ctx_hip(ctx, hipGetLastError(), what);
}

int launch_mlp_train_forward(dlrm_ctx* ctx, const dlrm_mlp_train_layout& L, const int* sizes, int batch, const void* x,
                             int x_dtype, int64_t x_ld, const float* const* b, const void* w16, void* acts, void* out,
                             int out_dtype, int64_t out_ld, bool last_relu) {
    int rc = mt_convert(ctx, x, x_dtype, x_ld, nullptr, 0, 0, mt_at(acts, L.a_off[0]), L.ld[0], mt_at(acts, L.at_off[0]),
                        L.ldt, batch, sizes[0]);
    for (int l = 0; l < L.layers && rc == DLRM_OK; ++l) {
        const bool last = l == L.layers - 1;
        MtGemmArgs a{};
        a.A = mt_at(w16, L.w_off[l]);
        a.B = mt_at(acts, L.a_off[l]);
        a.lda = a.ldb = L.ld[l];
        a.rowsA = sizes[l + 1];
        a.rowsB = batch;
        a.ksteps = a.per_slab = L.ld[l] / kMtTile;
        a.bias = b[l];
        a.relu = !last || last_relu;
        if (last) {
            a.fin = out;
            a.ld_fin = out_ld;
            a.fin_bf16 = out_dtype == DLRM_BF16;
        } else {
            a.out = mt_at(acts, L.a_off[l + 1]);
            a.outT = mt_at(acts, L.at_off[l + 1]);
            a.ld_out = L.ld[l + 1];
            a.ld_outT = L.ldt;
        }
        rc = mt_gemm<kMtFwd>(ctx, a, 1, "mlp_train_fwd launch");
    }
    return rc;
}

int launch_mlp_train_backward(dlrm_ctx* ctx, const dlrm_mlp_train_layout& L, const int* sizes, int batch, const void* dy,
                              int dy_dtype, int64_t dy_ld, const void* out, int out_dtype, int64_t out_ld,
                              const void* w16, const void* acts, void* grads, void* part, float* const* gW,
                              const int64_t* gw_ld, float* const* gb, bool write_last_gb, void* dx, int dx_dtype,
                              int64_t dx_ld) {
    const int n = L.layers, msteps = mt_ceil(batch, kMtTile) / kMtTile;
    int rc = mt_convert(ctx, dy, dy_dtype, dy_ld, out, out_dtype, out_ld, mt_at(grads, L.g_off[n - 1]), L.ld[n],
                        mt_at(grads, L.gt_off[n - 1]), L.ldt, batch, sizes[n]);
    MtReduceArgs red{};
    red.layers = n;
    for (int l = n - 1; l >= 0 && rc == DLRM_OK; --l) {  // layer l + 1: levels l -> l + 1
        const int K = sizes[l], N = sizes[l + 1];
        float* gbl = (l == n - 1 && !write_last_gb) ? nullptr : gb[l];
        int rows = 0;
        int slabs = mt_slabs((L.ld[l] / kMtTile) * (L.ld[l + 1] / kMtTile), msteps, &rows);
        if (slabs > L.slabs[l]) {  // (the rule is not monotone in the batch: never more slabs than the buffer holds)
            const int per = (msteps + L.slabs[l] - 1) / L.slabs[l];
            slabs = (msteps + per - 1) / per;
            rows = per * kMtTile;
        }
        MtGemmArgs a{};
        a.A = mt_at(grads, L.gt_off[l]);
        a.B = mt_at(acts, L.at_off[l]);
        a.lda = a.ldb = L.ldt;
        a.rowsA = N;
        a.rowsB = K;
        a.ksteps = msteps;
        a.per_slab = rows / kMtTile;
        a.gW = gW[l];
        a.ld_gw = gw_ld[l];
        a.gb = gbl;
        a.part = (float*)((char*)part + L.p_off[l]);
        a.partb = (float*)((char*)part + L.pb_off[l]);
        a.slabs = slabs;
        rc = mt_gemm<kMtWgrad>(ctx, a, slabs, "mlp_train_wgrad launch");
        red.part[l] = a.part;
        red.partb[l] = a.partb;
        red.gW[l] = gW[l];
        red.gb[l] = gbl;
        red.ld_gw[l] = gw_ld[l];
        red.N[l] = N;
        red.K[l] = K;
        red.slabs[l] = slabs;
        if (rc != DLRM_OK || (l == 0 && !dx)) continue;
        MtGemmArgs d{};
        d.A = mt_at(w16, L.wt_off[l]);
        d.B = mt_at(grads, L.g_off[l]);
        d.lda = d.ldb = L.ld[l + 1];
        d.rowsA = K;
        d.rowsB = batch;
        d.ksteps = d.per_slab = L.ld[l + 1] / kMtTile;
        if (l == 0) {
            d.fin = dx;
            d.ld_fin = dx_ld;
            d.fin_bf16 = dx_dtype == DLRM_BF16;
        } else {
            d.mask = mt_at(acts, L.a_off[l]);
            d.ld_mask = L.ld[l];
            d.out = mt_at(grads, L.g_off[l - 1]);
            d.outT = mt_at(grads, L.gt_off[l - 1]);
            d.ld_out = L.ld[l];
            d.ld_outT = L.ldt;
        }
        rc = mt_gemm<kMtDgrad>(ctx, d, 1, "mlp_train_dgrad launch");
    }
    if (rc != DLRM_OK) return rc;
    for (int l = 0; l < n; ++l)
        red.start[l + 1] = red.start[l] + (red.slabs[l] > 1 ? (int64_t)red.N[l] * red.K[l] + red.N[l] : 0);
    if (red.start[n] == 0) return DLRM_OK;
    hipLaunchKernelGGL(mlp_train_reduce_kernel, dim3(mt_blocks(ctx, red.start[n])), dim3(256), 0, ctx_stream(ctx), red);
    return ctx_hip(ctx, hipGetLastError(), "mlp_train_reduce launch");
}

}  // namespace dlrm
