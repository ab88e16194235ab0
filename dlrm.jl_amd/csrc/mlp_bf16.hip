// mlp_bf16.hip — inference forward of a Dense chain a_{l+1} = act_l(a_l W_l^T + b_l) in ONE launch on gfx950 MFMA.
//
// bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 accumulation and bias, hidden activations rounded to bf16 (ties to
// even) and kept in LDS: no activation touches HBM between the input and the last layer's output.
//
// Packed weights (mlp_bf16_pack_kernel, layout in mlp_plan.hpp): layer l is [Np/16][Kp/32][64 lanes][8 bf16]; lane
// (c = lane % 16, q = lane / 16) of block (nb, kb) holds W[16 nb + c][32 kb + 8q .. 8q + 7] -- the MFMA operand layout
// interact.hip documents -- so a wave's operand load is one contiguous 1 KB and needs no shuffle.
//
// Chain kernel: a workgroup of four waves owns MT (16 or 32) batch rows.  Two LDS buffers of MT x (wmax + 8) bf16;
// layer l reads buffer l % 2 and writes the other, one block barrier per layer.  The four waves split a layer's Np
// columns into 64-column chunks (four 16-row weight blocks), wave w taking chunks w, w + 4, ...  The operands are
// swapped -- the weights are the MFMA's first operand, the activations the second -- so D[n][m]: lane (c, q) ends with
// n = 16 nb + 4q .. 4q + 3 of sample m = c, which after bias and activation is one packed 8-B LDS store (hidden
// layers) or four masked global stores (last layer).  Activation operands are 16-B LDS reads of 8 consecutive k of
// row c (row stride = 16 B mod 32 B: conflict-free).  Weight operands stream from global memory (L2 / MALL) through a
// rolling window of D k-steps in registers: slot s % D holds step s, is refilled right after its MFMAs with step
// s + D, and in a layer's last D steps with the NEXT layer's first steps, so the stream does not drain at a barrier.
// Biases reach the epilogue through LDS (8 KB static beside the dynamic buffers), a layer ahead.
// A wave's steps are (chunk, kb) in order; a step is 4 operand loads (64 B per lane) and 4 MT/16 MFMAs.
// No atomics; every address is plain indexing.  Rows >= B are clamped on load and never stored.
#include "mlp_bf16.hpp"

namespace dlrm {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

constexpr int kMlpDepth = 8;  // k-steps of weights in flight per wave (8 x 64 B per lane)

// two fp32 -> two bf16 in one word, ties to even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){lo, hi}, bf16x2_t));
}

// -------------------------------------------------------------------------------------------------------- pack
struct MlpPackArgs {
    const float* W[kMlpMaxLayers];
    const float* b[kMlpMaxLayers];
    int64_t ld[kMlpMaxLayers];
    uint16_t* w[kMlpMaxLayers];  // packed weights of the layer
    float* bo[kMlpMaxLayers];    // padded bias of the layer
    int N[kMlpMaxLayers], K[kMlpMaxLayers], KB[kMlpMaxLayers], NB[kMlpMaxLayers];
    int64_t start[kMlpMaxLayers + 1];  // items before the layer: NB KB 64 lane vectors, then 16 NB bias words
    int layers;
};

__global__ __launch_bounds__(256) void mlp_bf16_pack_kernel(const MlpPackArgs a) {
    const int64_t total = a.start[a.layers];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int l = 0;
        while (l + 1 < a.layers && i >= a.start[l + 1]) ++l;
        const int j = (int)(i - a.start[l]);
        const int N = a.N[l], K = a.K[l], KB = a.KB[l], nvec = a.NB[l] * KB * 64;
        if (j < nvec) {
            const int lane = j & 63, blk = j >> 6, nb = blk / KB, kb = blk - nb * KB;
            const int n = nb * 16 + (lane & 15), k0 = kb * 32 + 8 * (lane >> 4);
            const float* row = a.W[l] + (int64_t)n * a.ld[l];
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (n < N && k0 + e < K) ? ldg<float>(row + k0 + e) : 0.0f;
            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
            const u32x4_t v = {pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]), pack_bf16(f[4], f[5]), pack_bf16(f[6], f[7])};
            stg<u32x4_t>(a.w[l] + (int64_t)j * 8, v);
        } else {
            const int n = j - nvec;
            stg<float>(a.bo[l] + n, n < N ? ldg<float>(a.b[l] + n) : 0.0f);
        }
    }
}

// ------------------------------------------------------------------------------------------------------- chain
struct MlpChainArgs {
    const uint16_t* w[kMlpMaxLayers];
    const float* b[kMlpMaxLayers];
    int KB[kMlpMaxLayers], NB[kMlpMaxLayers];
    int layers, K0, Kp0, N_last;
    int stride;  // LDS row stride in bf16 elements: wmax + kMlpRowPad
};

template <int MT, int D>
__global__ __launch_bounds__(kMlpThreads) void mlp_bf16_chain_kernel(const MlpChainArgs a, const void* x, int x_bf16,
                                                                     int64_t x_ld, int x_vec, void* out, int out_bf16,
                                                                     int64_t out_ld, int B, int last_relu) {
    extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
    // the layer's bias, by layer parity: LDS reads do not count against vmcnt, so an epilogue never waits on the
    // weight window (a global load there would drain it: loads return in order)
    __shared__ __attribute__((aligned(16))) float sbias[2][kMlpMaxWidth];
    static_assert(sizeof(sbias) == kMlpStaticLds, "mlp_plan.hpp counts this");
    constexpr int MB = MT / 16;
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: every branch on it is a scalar branch)
    const int row0 = blockIdx.x * MT, stride = a.stride;

    // this wave's k-steps of layer l: its chunks w, w + 4, ... times the layer's KB
    auto steps_of = [&](int l) {
        const int nch = (a.NB[l] + 3) >> 2;
        return w < nch ? ((nch - 1 - w) / 4 + 1) * a.KB[l] : 0;
    };
    // the four weight operands of step (ch, kb): blocks past the layer's last (a partial chunk) reload the last one
    auto load_step = [&](bf16x8_t (&dst)[4], const uint16_t* wp, int KB, int NB, int ch, int kb) {
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) {
            const int nb = min(ch * 4 + jn, NB - 1);
            dst[jn] = ldg<bf16x8_t>(wp + ((nb * KB + kb) * 64 + lane) * 8);
        }
    };
    // step `step` (< D) of layer l, found from the layer's start
    auto load_first = [&](bf16x8_t (&dst)[4], int l, int step) {
        const int KB = a.KB[l];
        int kb = step, ch = w;
        while (kb >= KB) { kb -= KB; ch += 4; }
        load_step(dst, a.w[l], KB, a.NB[l], ch, kb);
    };

    // a thread's share of a layer's padded bias: loaded a layer ahead, stored to sbias before the barrier
    constexpr int BPT = kMlpMaxWidth / kMlpThreads;
    auto bias_load = [&](float (&r)[BPT], int l) {
        const int np = a.NB[l] * 16;
#pragma unroll
        for (int i = 0; i < BPT; ++i) r[i] = ldg<float>(a.b[l] + min(tid + i * kMlpThreads, np - 1));
    };
    auto bias_store = [&](const float (&r)[BPT], int l) {
#pragma unroll
        for (int i = 0; i < BPT; ++i) sbias[l & 1][tid + i * kMlpThreads] = r[i];
    };

    bf16x8_t win[D][4];
    int ns = steps_of(0);
#pragma unroll
    for (int j = 0; j < D; ++j) load_first(win[j], 0, j);
    {
        float b0[BPT];
        bias_load(b0, 0);
        bias_store(b0, 0);
    }

    // the tile's input rows -> buffer 0 as bf16, 8 columns per item, columns K0 .. Kp0 zero
    {
        const int cpr = a.Kp0 >> 3, K0 = a.K0;
        for (int it = tid; it < MT * cpr; it += kMlpThreads) {
            const int r = it / cpr, col = (it - r * cpr) * 8;
            const int64_t gr = min(row0 + r, B - 1);
            const bool whole = x_vec && col + 8 <= K0;
            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
            u32x4_t v;
            if (x_bf16) {
                const uint16_t* xr = (const uint16_t*)x + gr * x_ld + col;
                if (whole) {
                    v = ldg<u32x4_t>(xr);
                } else {
                    uint32_t h[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) h[e] = col + e < K0 ? (uint32_t)ldg<uint16_t>(xr + e) : 0u;
                    v = u32x4_t{h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16};
                }
            } else {
                const float* xr = (const float*)x + gr * x_ld + col;
                float f[8];
                if (whole) {
                    const f32x4 lo = ldg<f32x4>(xr), hi = ldg<f32x4>(xr + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { f[e] = lo[e]; f[4 + e] = hi[e]; }
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = col + e < K0 ? ldg<float>(xr + e) : 0.0f;
                }
                v = u32x4_t{pack_bf16(f[0], f[1]), pack_bf16(f[2], f[3]), pack_bf16(f[4], f[5]), pack_bf16(f[6], f[7])};
            }
            *(u32x4_t*)(lds + r * stride + col) = v;
        }
    }
    __syncthreads();

    for (int l = 0; l < a.layers; ++l) {
        const bool last = l == a.layers - 1;
        const bool relu = !last || last_relu;
        const int KB = a.KB[l], NB = a.NB[l];
        const uint16_t* wp = a.w[l];
        const float* bp = sbias[l & 1];
        const int ns_next = last ? 0 : steps_of(l + 1);
        const int ln = last ? l : l + 1;  // the layer the window rolls onto
        const uint16_t* wpn = a.w[ln];
        const int KBn = a.KB[ln], NBn = a.NB[ln];
        int fch[D], fkb[D];  // its first D steps
#pragma unroll
        for (int j = 0; j < D; ++j) {
            int kb = j, ch = w;
            while (kb >= KBn) { kb -= KBn; ch += 4; }
            fch[j] = ch;
            fkb[j] = kb;
        }
        float bnext[BPT];
        bias_load(bnext, ln);
        const uint16_t* in = lds + (l & 1) * MT * stride;
        uint16_t* ob = lds + ((l & 1) ^ 1) * MT * stride;

        f32x4 acc[4][MB];
        auto clear = [&]() {
#pragma unroll
            for (int jn = 0; jn < 4; ++jn)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) acc[jn][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
        };
        // the activation operands of k-step kb: 8 consecutive k of row 16 mb + c
        auto lds_read = [&](bf16x8_t (&bv)[MB], int kb) {
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) bv[mb] = *(const bf16x8_t*)(in + (mb * 16 + c) * stride + kb * 32 + 8 * q);
        };
        // chunk ch is complete: bias, activation, and the four n of this lane's sample go out together
        auto epilogue = [&](int ch) {
#pragma unroll
            for (int jn = 0; jn < 4; ++jn) {
                const int nb = ch * 4 + jn;
                if (nb >= NB) continue;
                const int n0 = nb * 16 + 4 * q;
                const f32x4 bias = *(const f32x4*)(bp + n0);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    f32x4 v = acc[jn][mb] + bias;
                    if (relu) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = v[r] < 0.0f ? 0.0f : v[r];
                    }
                    const int m = mb * 16 + c;
                    if (!last) {
                        *(u32x2_t*)(ob + m * stride + n0) = u32x2_t{pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])};
                    } else if (row0 + m < B) {
                        const int64_t o = (int64_t)(row0 + m) * out_ld + n0;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (n0 + r >= a.N_last) continue;
                            if (out_bf16) stg<uint16_t>((uint16_t*)out + o + r, (uint16_t)(pack_bf16(v[r], 0.0f) & 0xffffu));
                            else stg<float>((float*)out + o + r, v[r]);
                        }
                    }
                }
            }
        };

        int lkb = D, lch = w;  // the refill's cursor: step s + D of this layer
        while (lkb >= KB) { lkb -= KB; lch += 4; }
        int ckb = 0, cch = w;  // the MFMAs' cursor
        bf16x8_t bcur[MB], bnxt[MB];
        clear();
        if (ns > 0) lds_read(bcur, 0);
        // Every layer visits every slot at least once, and every visit refills its slot, whether or not the visit
        // is a step of this wave (s < ns): the loads in flight are then the same count on every path, which is what
        // lets the compiler wait for a slot with vmcnt(4 (D - 1)) and not drain the window.  The refill is this
        // layer's step s + D, else the next layer's step j (a step that does not exist reloads a block that does:
        // load_step clamps).
        for (int s0 = 0; s0 < max(ns, 1); s0 += D) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const int s = s0 + j;
                if (s < ns) {
                    const int nkb = ckb + 1 == KB ? 0 : ckb + 1;
                    lds_read(bnxt, nkb);  // (after the layer's last step: k-step 0 again, unused)
#pragma unroll
                    for (int jn = 0; jn < 4; ++jn)
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb)
                            acc[jn][mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(win[j][jn], bcur[mb], acc[jn][mb], 0, 0, 0);
                    if (nkb == 0) {
                        epilogue(cch);
                        clear();
                        cch += 4;
                    }
                    ckb = nkb;
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) bcur[mb] = bnxt[mb];
                }
                const bool cur = s + D < ns;
                load_step(win[j], cur ? wp : wpn, cur ? KB : KBn, cur ? NB : NBn, cur ? lch : fch[j], cur ? lkb : fkb[j]);
                if (cur && ++lkb == KB) { lkb = 0; lch += 4; }
            }
        }
        // columns Np .. Kp of the next layer's input (Np = 16 mod 32) are zero
        if (!last && (NB & 1) && tid < MT * 2) {
            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
            *(u32x4_t*)(ob + (tid >> 1) * stride + NB * 16 + 8 * (tid & 1)) = u32x4_t{0u, 0u, 0u, 0u};
        }
        if (!last) bias_store(bnext, l + 1);
        __syncthreads();
        ns = ns_next;
    }
}

// ---------------------------------------------------------------------------------------------------- launchers
int mlp_bf16_prepare(dlrm_ctx* ctx) {
    int rc = ctx_hip(ctx, hipFuncSetAttribute((const void*)mlp_bf16_chain_kernel<16, kMlpDepth>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, kMlpLdsMax - kMlpStaticLds),
                     "hipFuncSetAttribute(mlp_bf16_chain<16>)");
    if (rc != DLRM_OK) return rc;
    return ctx_hip(ctx, hipFuncSetAttribute((const void*)mlp_bf16_chain_kernel<32, kMlpDepth>,
                                            hipFuncAttributeMaxDynamicSharedMemorySize, kMlpLdsMax - kMlpStaticLds),
                   "hipFuncSetAttribute(mlp_bf16_chain<32>)");
}

int launch_mlp_bf16_pack(dlrm_ctx* ctx, const MlpPlan& p, void* packed, const float* const* W, const int64_t* w_ld,
                         const float* const* b) {
    MlpPackArgs a{};
    a.layers = p.layers;
    a.start[0] = 0;
    for (int l = 0; l < p.layers; ++l) {
        a.W[l] = W[l];
        a.b[l] = b[l];
        a.ld[l] = w_ld[l];
        a.w[l] = (uint16_t*)((char*)packed + p.w_off[l]);
        a.bo[l] = (float*)((char*)packed + p.b_off[l]);
        a.N[l] = p.N[l];
        a.K[l] = p.K[l];
        a.KB[l] = p.Kp[l] / 32;
        a.NB[l] = p.Np[l] / 16;
        a.start[l + 1] = a.start[l] + (int64_t)a.NB[l] * a.KB[l] * 64 + p.Np[l];
    }
    const int64_t blocks = (a.start[p.layers] + 255) / 256;
    const int cap = ctx_num_cus(ctx) * 8;
    hipLaunchKernelGGL(mlp_bf16_pack_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, ctx_stream(ctx), a);
    return ctx_hip(ctx, hipGetLastError(), "mlp_bf16_pack launch");
}

int launch_mlp_bf16_chain(dlrm_ctx* ctx, const MlpPlan& p, const void* packed, int batch, const void* x, int x_dtype,
                          int64_t x_ld, void* out, int out_dtype, int64_t out_ld, bool last_relu) {
    if (batch == 0) return DLRM_OK;
    MlpChainArgs a{};
    a.layers = p.layers;
    for (int l = 0; l < p.layers; ++l) {
        a.w[l] = (const uint16_t*)((const char*)packed + p.w_off[l]);
        a.b[l] = (const float*)((const char*)packed + p.b_off[l]);
        a.KB[l] = p.Kp[l] / 32;
        a.NB[l] = p.Np[l] / 16;
    }
    a.K0 = p.K[0];
    a.Kp0 = p.Kp[0];
    a.N_last = p.N[p.layers - 1];
    a.stride = p.wmax + kMlpRowPad;
    const int xb = x_dtype == DLRM_BF16, ob = out_dtype == DLRM_BF16;
    const int x_vec = (uintptr_t)x % 16 == 0 && (x_ld * (xb ? 2 : 4)) % 16 == 0;
    hipStream_t s = ctx_stream(ctx);
    if (p.MT == 16)
        hipLaunchKernelGGL((mlp_bf16_chain_kernel<16, kMlpDepth>), dim3(p.grid), dim3(kMlpThreads), (size_t)p.lds_bytes, s, a,
                           x, xb, x_ld, x_vec, out, ob, out_ld, batch, (int)last_relu);
    else
        hipLaunchKernelGGL((mlp_bf16_chain_kernel<32, kMlpDepth>), dim3(p.grid), dim3(kMlpThreads), (size_t)p.lds_bytes, s, a,
                           x, xb, x_ld, x_vec, out, ob, out_ld, batch, (int)last_relu);
    return ctx_hip(ctx, hipGetLastError(), "mlp_bf16_chain launch");
}

}  // namespace dlrm
