// mlp_fp8.hip — inference forward of a Dense chain a_{l+1} = act_l(a_l W_l^T + b_l) in ONE launch on the block-scaled
// fp8 MFMA of gfx950 (v_mfma_scale_f32_16x16x128_f8f6f4): OCP MXFP8, e4m3 codes with one E8M0 scale per 32
// consecutive k of a row, fp32 accumulation and bias.
//
// Quantisation of a block v[0..31] (OCP MX v1.0): m = max |v|; the scale byte is max(exponent_field(m) - 8, 0), that
// is X + 127 with X = clamp(floor(log2 m) - 8, -127, 127) (0 for a zero block); a code is RNE_e4m3(v 2^-X) after a
// clamp to +-448 in fp32 (v_med3), so the conversion never sees a value it could overflow on.
//
// Packed weights (mlp_fp8_pack_kernel, layout in mlp_fp8_plan.hpp): codes [Np/16][Kp/128][64 lanes][32 B], lane
// (c = lane % 16, q = lane / 16) of block (nb, kb) holding W[16 nb + c][128 kb + 32 q .. + 31]; scale bytes
// [Np/16][Kp/128][64 lanes], the lane's own row and its own 32 elements.  A wave's operand load is one contiguous
// 2 KB (two 16-B loads per lane) and its scale load one contiguous 64 B.
//
// Chain kernel: a workgroup of four waves owns MT (16, 32 or 64) batch rows.  LDS holds two alternating activation
// buffers of MT x (wmax + 16) code bytes and MT x wmax / 32 scale bytes; layer l reads buffer l % 2 and writes the
// other, one block barrier per layer.  The input rows are quantised on load, a thread per (row, block of 32).  The
// four waves split a layer's Np columns into 64-column chunks (four 16-row weight blocks), wave w taking chunks
// w, w + 4, ...; a k-step is 128 k: four weight operands (32 B per lane each) with their scale bytes from global
// memory, MT/16 activation operands (two ds_read_b128 each; the row stride is 16 B off a multiple of 128 B, so the
// 16 rows of a read cover the 64 banks once) with their scale bytes from LDS, and 4 MT/16 MFMAs.  The weights are
// the first operand, the activations the second: D[n][m], lane (c, q) ends with n = 16 nb + 4q .. 4q + 3 of sample
// m = c.  A 32-feature scale block of the next layer's input is then two accumulators (n-blocks 2j, 2j + 1) times
// the four q lanes of one c: bias, relu, a max over the lane's eight values, two cross-lane steps over q, the
// exponent, the scaling (v_ldexp, exact), the clamp, the conversion and one packed 4-B store per n-block, plus one
// scale byte per block by the q = 0 lane.  No LDS round trip for the maximum.
// Weights stream through a rolling window of D k-steps in registers: slot s % D holds step s of the wave's
// (chunk, kb) sequence and is refilled right after its MFMAs with step s + D.  Every visit refills (past the layer's
// last step: that step again), so the loads in flight are the same count on every path and a slot is awaited with a
// non-zero vmcnt.  The window is primed at a layer's start; it does not roll across the barrier.  Biases reach the
// epilogue through LDS (8 KB static), a layer ahead, so no epilogue waits on the window.
// No atomics; every address is plain indexing.  Rows >= B are clamped on load and never stored.
#include "mlp_fp8.hpp"

namespace dlrm {

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

constexpr int kFp8Depth = 4;  // k-steps of weights in flight per wave (4 x 128 B per lane)

// the E8M0 byte of a block whose largest magnitude is m (finite, >= 0)
__device__ __forceinline__ int mx_scale_byte(float m) {
    const int e = (int)((__builtin_bit_cast(uint32_t, m) >> 23) & 0xffu);
    return max(e - 8, 0);
}
// v 2^-X (exact) clamped to the e4m3 range, for the block's byte X + 127
__device__ __forceinline__ float mx_scaled(float v, int byte) {
    return __builtin_amdgcn_fmed3f(ldexpf(v, 127 - byte), -448.0f, 448.0f);
}
// four fp32 -> four e4m3 codes in one word, ties to even (v_cvt_pk_fp8_f32)
__device__ __forceinline__ uint32_t pack_fp8x4(float a, float b, float c, float d) {
    const int lo = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c, d, lo, true);
}
// a block of 32 fp32 values -> its byte and its 32 codes
__device__ __forceinline__ int mx_quantize_block(const float (&f)[32], u32x4_t& lo, u32x4_t& hi) {
    float m = 0.0f;
#pragma unroll
    for (int e = 0; e < 32; ++e) m = fmaxf(m, fabsf(f[e]));
    const int byte = mx_scale_byte(m);
    uint32_t d[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
        d[e] = pack_fp8x4(mx_scaled(f[4 * e], byte), mx_scaled(f[4 * e + 1], byte), mx_scaled(f[4 * e + 2], byte),
                          mx_scaled(f[4 * e + 3], byte));
    lo = u32x4_t{d[0], d[1], d[2], d[3]};
    hi = u32x4_t{d[4], d[5], d[6], d[7]};
    return byte;
}
__device__ __forceinline__ uint16_t bf16_bits(float v) {
    return (uint16_t)(__builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){v, 0.0f}, bf16x2_t)) & 0xffffu);
}

// -------------------------------------------------------------------------------------------------------- pack
struct Fp8PackArgs {
    const float* W[kFp8MaxLayers];
    const float* b[kFp8MaxLayers];
    int64_t ld[kFp8MaxLayers];
    uint8_t* w[kFp8MaxLayers];  // packed codes of the layer
    uint8_t* s[kFp8MaxLayers];  // their scale bytes
    float* bo[kFp8MaxLayers];   // padded bias of the layer
    int N[kFp8MaxLayers], K[kFp8MaxLayers], KB[kFp8MaxLayers], NB[kFp8MaxLayers];
    int64_t start[kFp8MaxLayers + 1];  // items before the layer: NB KB 64 lane blocks, then 16 NB bias words
    int layers;
};

__global__ __launch_bounds__(256) void mlp_fp8_pack_kernel(const Fp8PackArgs a) {
    const int64_t total = a.start[a.layers];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        int l = 0;
        while (l + 1 < a.layers && i >= a.start[l + 1]) ++l;
        const int j = (int)(i - a.start[l]);
        const int N = a.N[l], K = a.K[l], KB = a.KB[l], nblk = a.NB[l] * KB * 64;
        if (j < nblk) {
            const int lane = j & 63, blk = j >> 6, nb = blk / KB, kb = blk - nb * KB;
            const int n = nb * 16 + (lane & 15), k0 = kb * 128 + 32 * (lane >> 4);
            const float* row = a.W[l] + (int64_t)n * a.ld[l];
            float f[32];
#pragma unroll
            for (int e = 0; e < 32; ++e) f[e] = (n < N && k0 + e < K) ? ldg<float>(row + k0 + e) : 0.0f;
            u32x4_t lo, hi;
            const int byte = mx_quantize_block(f, lo, hi);
            stg<u32x4_t>(a.w[l] + (int64_t)j * 32, lo);
            stg<u32x4_t>(a.w[l] + (int64_t)j * 32 + 16, hi);
            stg<uint8_t>(a.s[l] + j, (uint8_t)byte);
        } else {
            const int n = j - nblk;
            stg<float>(a.bo[l] + n, n < N ? ldg<float>(a.b[l] + n) : 0.0f);
        }
    }
}

// ------------------------------------------------------------------------------------------------------- chain
struct Fp8ChainArgs {
    const uint8_t* w[kFp8MaxLayers];
    const uint8_t* s[kFp8MaxLayers];
    const float* b[kFp8MaxLayers];
    int KB[kFp8MaxLayers], NB[kFp8MaxLayers];
    int layers, K0, Kp0, N_last;
    int stride;   // LDS code row stride in bytes: wmax + kFp8RowPad
    int sstride;  // LDS scale row stride in bytes: wmax / 32
};

template <int MT, int D>
__global__ __launch_bounds__(kFp8Threads) void mlp_fp8_chain_kernel(const Fp8ChainArgs a, const void* x, int x_bf16,
                                                                    int64_t x_ld, int x_vec, void* out, int out_bf16,
                                                                    int64_t out_ld, int B, int last_relu) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds8[];
    // the layer's bias, by layer parity: LDS reads do not count against vmcnt, so an epilogue never waits on the
    // weight window
    __shared__ __attribute__((aligned(16))) float sbias[2][kFp8MaxWidth];
    static_assert(sizeof(sbias) == kFp8StaticLds, "mlp_fp8_plan.hpp counts this");
    constexpr int MB = MT / 16;
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // (scalar: every branch on it is a scalar branch)
    const int row0 = blockIdx.x * MT, stride = a.stride, sstride = a.sstride;
    // The instruction's own k order: a lane's registers 0-3 are k = 16 q .. + 15 of the k-step and its registers 4-7
    // k = 64 + 16 q .. + 15, while its scale is that of k = 32 q .. + 31.  In the packed block (a piece of 32 B per
    // (c, 32 k)) the lane's low half is bytes 16 (q & 1) .. of piece (c, q / 2), its high half those of piece
    // (c, 2 + q / 2): still two 16-B loads inside the block's contiguous 2 KB.
    const int koff = (q >> 1) * 16 + c;
    uint8_t* const codes = lds8;                      // [2][MT][stride]
    uint8_t* const scales = lds8 + 2 * MT * stride;   // [2][MT][sstride]

    // a thread's share of a layer's padded bias: loaded a layer ahead, stored to sbias before the barrier
    constexpr int BPT = kFp8MaxWidth / kFp8Threads;
    auto bias_load = [&](float (&r)[BPT], int l) {
        const int np = a.NB[l] * 16;
#pragma unroll
        for (int i = 0; i < BPT; ++i) r[i] = ldg<float>(a.b[l] + min(tid + i * kFp8Threads, np - 1));
    };
    auto bias_store = [&](const float (&r)[BPT], int l) {
#pragma unroll
        for (int i = 0; i < BPT; ++i) sbias[l & 1][tid + i * kFp8Threads] = r[i];
    };
    {
        float b0[BPT];
        bias_load(b0, 0);
        bias_store(b0, 0);
    }

    // the tile's input rows -> buffer 0 as MXFP8, a (row, block of 32 columns) per item, columns K0 .. Kp0 zero
    {
        const int bpr = a.Kp0 >> 5, K0 = a.K0;
        for (int it = tid; it < MT * bpr; it += kFp8Threads) {
            const int r = it / bpr, blk = it - r * bpr, col = blk * 32;
            const int64_t gr = min(row0 + r, B - 1);
            const bool whole = x_vec && col + 32 <= K0;
            float f[32];
            if (x_bf16) {
                const uint16_t* xr = (const uint16_t*)x + gr * x_ld + col;
                if (whole) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const u16x8 h = ldg<u16x8>(xr + 8 * v);
#pragma unroll
                        for (int e = 0; e < 8; ++e) f[8 * v + e] = __builtin_bit_cast(float, (uint32_t)h[e] << 16);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 32; ++e)
                        f[e] = col + e < K0 ? __builtin_bit_cast(float, (uint32_t)ldg<uint16_t>(xr + e) << 16) : 0.0f;
                }
            } else {
                const float* xr = (const float*)x + gr * x_ld + col;
                if (whole) {
#pragma unroll
                    for (int v = 0; v < 8; ++v) {
                        const f32x4 t = ldg<f32x4>(xr + 4 * v);
#pragma unroll
                        for (int e = 0; e < 4; ++e) f[4 * v + e] = t[e];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 32; ++e) f[e] = col + e < K0 ? ldg<float>(xr + e) : 0.0f;
                }
            }
            u32x4_t lo, hi;
            const int byte = mx_quantize_block(f, lo, hi);
            *(u32x4_t*)(codes + r * stride + col) = lo;
            *(u32x4_t*)(codes + r * stride + col + 16) = hi;
            scales[r * sstride + blk] = (uint8_t)byte;
        }
    }
    __syncthreads();

    for (int l = 0; l < a.layers; ++l) {
        const bool last = l == a.layers - 1;
        const bool relu = !last || last_relu;
        const int KB = a.KB[l], NB = a.NB[l];
        const uint8_t* wp = a.w[l];
        const uint8_t* sp = a.s[l];
        const float* bp = sbias[l & 1];
        float bnext[BPT];
        bias_load(bnext, last ? l : l + 1);
        const uint8_t* in = codes + (l & 1) * MT * stride;
        const uint8_t* insc = scales + (l & 1) * MT * sstride;
        uint8_t* ob = codes + ((l & 1) ^ 1) * MT * stride;
        uint8_t* obsc = scales + ((l & 1) ^ 1) * MT * sstride;
        // this wave's k-steps: its chunks w, w + 4, ... times KB
        const int nch = (NB + 3) >> 2;
        const int ns = w < nch ? ((nch - 1 - w) / 4 + 1) * KB : 0;

        if (ns > 0) {
            // the four weight operands and scale bytes of step (ch, kb): blocks past the layer's last (a partial
            // chunk) reload the last one
            i32x8_t win[D][4];
            int wsc[D][4];
            auto load_step = [&](i32x8_t (&dst)[4], int (&sc)[4], int ch, int kb) {
#pragma unroll
                for (int jn = 0; jn < 4; ++jn) {
                    const int nb = min(ch * 4 + jn, NB - 1);
                    const int o = (nb * KB + kb) * 64;
                    const i32x4_t lo = ldg<i32x4_t>(wp + (o + koff) * 32 + 16 * (q & 1));
                    const i32x4_t hi = ldg<i32x4_t>(wp + (o + koff + 32) * 32 + 16 * (q & 1));
                    dst[jn] = i32x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    sc[jn] = (int)ldg<uint8_t>(sp + o + lane);
                }
            };
            int ls = 0, lkb = 0, lch = w;  // the refill's cursor: step ls, held at the layer's last step
            auto advance = [&]() {
                if (ls + 1 < ns) {
                    ++ls;
                    if (++lkb == KB) { lkb = 0; lch += 4; }
                }
            };
#pragma unroll
            for (int j = 0; j < D; ++j) {
                load_step(win[j], wsc[j], lch, lkb);
                advance();
            }

            f32x4 acc[4][MB];
            auto clear = [&]() {
#pragma unroll
                for (int jn = 0; jn < 4; ++jn)
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) acc[jn][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
            };
            // the activation operands of k-step kb: 32 consecutive k of row 16 mb + c, and their scale byte
            auto lds_read = [&](i32x8_t (&bv)[MB], int (&bs)[MB], int kb) {
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const uint8_t* p = in + (mb * 16 + c) * stride + kb * 128 + 16 * q;
                    const i32x4_t lo = *(const i32x4_t*)p, hi = *(const i32x4_t*)(p + 64);
                    bv[mb] = i32x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    bs[mb] = (int)insc[(mb * 16 + c) * sstride + kb * 4 + q];
                }
            };
            // chunk ch is complete.  Hidden layer: a pair of n-blocks is one scale block of the next layer's input.
            auto epilogue = [&](int ch) {
#pragma unroll
                for (int jp = 0; jp < 2; ++jp) {
                    const int nb = ch * 4 + 2 * jp;
                    if (nb >= NB) continue;
                    const bool two = nb + 1 < NB;
                    const int n0 = nb * 16 + 4 * q;
                    const f32x4 bias0 = *(const f32x4*)(bp + n0);
                    const f32x4 bias1 = two ? *(const f32x4*)(bp + n0 + 16) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
                        f32x4 v0 = acc[2 * jp][mb] + bias0;
                        f32x4 v1 = two ? acc[2 * jp + 1][mb] + bias1 : f32x4{0.f, 0.f, 0.f, 0.f};
                        if (relu) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                v0[r] = v0[r] < 0.0f ? 0.0f : v0[r];
                                v1[r] = v1[r] < 0.0f ? 0.0f : v1[r];
                            }
                        }
                        const int m = mb * 16 + c;
                        if (!last) {
                            float mx = fmaxf(fmaxf(fmaxf(v0[0], v0[1]), fmaxf(v0[2], v0[3])),
                                             fmaxf(fmaxf(v1[0], v1[1]), fmaxf(v1[2], v1[3])));  // (relu'd: >= 0)
                            mx = fmaxf(mx, __shfl_xor(mx, 16));
                            mx = fmaxf(mx, __shfl_xor(mx, 32));
                            const int byte = mx_scale_byte(mx);
                            *(uint32_t*)(ob + m * stride + n0) = pack_fp8x4(mx_scaled(v0[0], byte), mx_scaled(v0[1], byte),
                                                                            mx_scaled(v0[2], byte), mx_scaled(v0[3], byte));
                            if (two)
                                *(uint32_t*)(ob + m * stride + n0 + 16) = pack_fp8x4(
                                    mx_scaled(v1[0], byte), mx_scaled(v1[1], byte), mx_scaled(v1[2], byte), mx_scaled(v1[3], byte));
                            if (q == 0) obsc[m * sstride + (nb >> 1)] = (uint8_t)byte;
                        } else if (row0 + m < B) {
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                if (h && !two) continue;
                                const f32x4 v = h ? v1 : v0;
                                const int64_t o = (int64_t)(row0 + m) * out_ld + n0 + 16 * h;
#pragma unroll
                                for (int r = 0; r < 4; ++r) {
                                    if (n0 + 16 * h + r >= a.N_last) continue;
                                    if (out_bf16) stg<uint16_t>((uint16_t*)out + o + r, bf16_bits(v[r]));
                                    else stg<float>((float*)out + o + r, v[r]);
                                }
                            }
                        }
                    }
                }
            };

            int ckb = 0, cch = w;  // the MFMAs' cursor
            i32x8_t bcur[MB], bnxt[MB];
            int scur[MB], snxt[MB];
            clear();
            lds_read(bcur, scur, 0);
            for (int s0 = 0; s0 < ns; s0 += D) {
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    if (s0 + j < ns) {
                        const int nkb = ckb + 1 == KB ? 0 : ckb + 1;
                        lds_read(bnxt, snxt, nkb);  // (after the layer's last step: k-step 0 again, unused)
#pragma unroll
                        for (int jn = 0; jn < 4; ++jn)
#pragma unroll
                            for (int mb = 0; mb < MB; ++mb)
                                acc[jn][mb] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                                    win[j][jn], bcur[mb], acc[jn][mb], 0, 0, 0, wsc[j][jn], 0, scur[mb]);
                        if (nkb == 0) {
                            epilogue(cch);
                            clear();
                            cch += 4;
                        }
                        ckb = nkb;
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) { bcur[mb] = bnxt[mb]; scur[mb] = snxt[mb]; }
                    }
                    load_step(win[j], wsc[j], lch, lkb);
                    advance();
                }
            }
        }
        if (!last) {
            // columns Np .. Kp of the next layer's input are zero codes, and their whole blocks zero bytes
            const int Np = NB * 16, Kpn = a.KB[l + 1] * 128;
            const int zc = (Kpn - Np) >> 4;
            for (int it = tid; it < MT * zc; it += kFp8Threads) {
                const int r = it / zc, j = it - r * zc;
                *(u32x4_t*)(ob + r * stride + Np + 16 * j) = u32x4_t{0u, 0u, 0u, 0u};
            }
            const int sb0 = (Np + 31) >> 5, zs = (Kpn >> 5) - sb0;
            for (int it = tid; it < MT * zs; it += kFp8Threads) {
                const int r = it / zs, j = it - r * zs;
                obsc[r * sstride + sb0 + j] = 0;
            }
            bias_store(bnext, l + 1);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------- launchers
template <int MT>
static int fp8_raise_lds(dlrm_ctx* ctx) {
    return ctx_hip(ctx, hipFuncSetAttribute((const void*)mlp_fp8_chain_kernel<MT, kFp8Depth>,
                                            hipFuncAttributeMaxDynamicSharedMemorySize, kFp8LdsMax - kFp8StaticLds),
                   "hipFuncSetAttribute(mlp_fp8_chain)");
}

int mlp_fp8_prepare(dlrm_ctx* ctx) {
    int rc = fp8_raise_lds<16>(ctx);
    if (rc == DLRM_OK) rc = fp8_raise_lds<32>(ctx);
    if (rc == DLRM_OK) rc = fp8_raise_lds<64>(ctx);
    return rc;
}

int launch_mlp_fp8_pack(dlrm_ctx* ctx, const MlpFp8Plan& p, void* packed, const float* const* W, const int64_t* w_ld,
                        const float* const* b) {
    Fp8PackArgs a{};
    a.layers = p.layers;
    a.start[0] = 0;
    for (int l = 0; l < p.layers; ++l) {
        a.W[l] = W[l];
        a.b[l] = b[l];
        a.ld[l] = w_ld[l];
        a.w[l] = (uint8_t*)packed + p.w_off[l];
        a.s[l] = (uint8_t*)packed + p.s_off[l];
        a.bo[l] = (float*)((char*)packed + p.b_off[l]);
        a.N[l] = p.N[l];
        a.K[l] = p.K[l];
        a.KB[l] = p.Kp[l] / 128;
        a.NB[l] = p.Np[l] / 16;
        a.start[l + 1] = a.start[l] + (int64_t)a.NB[l] * a.KB[l] * 64 + p.Np[l];
    }
    const int64_t blocks = (a.start[p.layers] + 255) / 256;
    const int cap = ctx_num_cus(ctx) * 8;
    hipLaunchKernelGGL(mlp_fp8_pack_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, ctx_stream(ctx), a);
    return ctx_hip(ctx, hipGetLastError(), "mlp_fp8_pack launch");
}

int launch_mlp_fp8_chain(dlrm_ctx* ctx, const MlpFp8Plan& p, const void* packed, int batch, const void* x, int x_dtype,
                         int64_t x_ld, void* out, int out_dtype, int64_t out_ld, bool last_relu) {
    if (batch == 0) return DLRM_OK;
    Fp8ChainArgs a{};
    a.layers = p.layers;
    for (int l = 0; l < p.layers; ++l) {
        a.w[l] = (const uint8_t*)packed + p.w_off[l];
        a.s[l] = (const uint8_t*)packed + p.s_off[l];
        a.b[l] = (const float*)((const char*)packed + p.b_off[l]);
        a.KB[l] = p.Kp[l] / 128;
        a.NB[l] = p.Np[l] / 16;
    }
    a.K0 = p.K[0];
    a.Kp0 = p.Kp[0];
    a.N_last = p.N[p.layers - 1];
    a.stride = p.wmax + kFp8RowPad;
    a.sstride = p.wmax / 32;
    const int xb = x_dtype == DLRM_BF16, ob = out_dtype == DLRM_BF16;
    const int x_vec = (uintptr_t)x % 16 == 0 && (x_ld * (xb ? 2 : 4)) % 16 == 0;
    hipStream_t s = ctx_stream(ctx);
    const dim3 grid(p.grid), block(kFp8Threads);
    const size_t lds = (size_t)p.lds_bytes;
    if (p.MT == 16)
        hipLaunchKernelGGL((mlp_fp8_chain_kernel<16, kFp8Depth>), grid, block, lds, s, a, x, xb, x_ld, x_vec, out, ob,
                           out_ld, batch, (int)last_relu);
    else if (p.MT == 32)
        hipLaunchKernelGGL((mlp_fp8_chain_kernel<32, kFp8Depth>), grid, block, lds, s, a, x, xb, x_ld, x_vec, out, ob,
                           out_ld, batch, (int)last_relu);
    else
        hipLaunchKernelGGL((mlp_fp8_chain_kernel<64, kFp8Depth>), grid, block, lds, s, a, x, xb, x_ld, x_vec, out, ob,
                           out_ld, batch, (int)last_relu);
    return ctx_hip(ctx, hipGetLastError(), "mlp_fp8_chain launch");
}

}  // namespace dlrm
