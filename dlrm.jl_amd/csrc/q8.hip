// q8.hip — int8 row-quantized embedding tables for inference and evaluation on gfx950.
//
// Format (include/dlrm_hip.h): table t is codes q[N_t][D] (uint8, row-major) and
// sb[N_t] = {scale, bias} (float2), two caller-owned arrays.  Per row w[0..D), every operation a separately
// rounded fp32 operation:
//   lo = min w, hi = max w, range = hi - lo, scale = range / 255, inv = range > 0 ? 255 / range : 0
//   q[c] = min(255, max(0, rint((w[c] - lo) * inv)))   (ties to even),   bias = lo
//   v[c] = (q[c] * scale) + bias                        (two roundings, never an fma: q8_value)
// A bf16 consumer gets f32_to_bf16(v[c]).
//
// Kernels: the quantizer (one lane group per row, streaming), the dequantizer (the way back, and every test's
// yardstick), the dequantizing gather (dlrm_maplookup on quantized rows) and the fused one-hot lookup + interaction
// forward, which writes the bits that the gather + interact.hip's forward write: the same MFMA lane layout
// (fwd_onehot.hpp: lane (c, q) holds columns step * COLS + q * PER_LANE .. of row 16 I + c) and the same
// even / odd column-step partials.
#include <type_traits>

#include "fwd_onehot.hpp"
#include "q8.hpp"

namespace dlrm {

// q * scale + bias in two roundings.  The library is built with -ffp-contract=fast, which fuses a multiply into a
// dependent add whatever a pragma says; the empty asm makes the product a value the combiner cannot look through
// (no instruction is emitted for it).
__device__ __forceinline__ float q8_value(float code, float scale, float bias) {
    float p = code * scale;
    asm("" : "+v"(p));
    return p + bias;
}

__device__ __forceinline__ uint32_t q8_code(float w, float lo, float inv) {
    return (uint32_t)fminf(255.0f, fmaxf(0.0f, rintf((w - lo) * inv)));
}

__device__ __forceinline__ Q8Desc load_q8(const Q8Desc* tabs, int t) {
    const uint4 a = ldg<uint4>(tabs + t), b = ldg<uint4>((const uint4*)(tabs + t) + 1);
    Q8Desc d;
    d.q = (uint8_t*)(((uint64_t)a.y << 32) | a.x);
    d.sb = (float2*)(((uint64_t)a.w << 32) | a.z);
    d.nrows = (int64_t)(((uint64_t)b.y << 32) | b.x);
    d.row0 = (int64_t)(((uint64_t)b.w << 32) | b.z);
    return d;
}

// The table that holds row r of the concatenated row range: the last t with row0[t] <= r (empty tables share
// their successor's row0 and are passed over).
__device__ __forceinline__ int q8_find_table(const Q8Desc* tabs, int ntab, int64_t r) {
    int lo = 0, hi = ntab;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ldg<int64_t>(&tabs[mid].row0) <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// E codes of a row from / to memory: 16 as one 16-B access (VEC), else one
template <int E> __device__ __forceinline__ void q8_load_codes(const uint8_t* p, float* f) {
    if constexpr (E == 16) {
        const uint4 u = ldg<uint4>(p);
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) f[k] = (float)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
    } else {
        f[0] = (float)ldg<uint8_t>(p);
    }
}
template <int E> __device__ __forceinline__ void q8_store_codes(uint8_t* p, const uint32_t* code) {
    if constexpr (E == 16) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w[k] = code[4 * k] | (code[4 * k + 1] << 8) | (code[4 * k + 2] << 16) | (code[4 * k + 3] << 24);
        stg<uint4>(p, uint4{w[0], w[1], w[2], w[3]});
    } else {
        stg<uint8_t>(p, (uint8_t)code[0]);
    }
}

// ---------------------------------------------------------------------------- quantizer
// One group of G lanes (a power of two, G * E >= D where that fits a wave) per row, 64 / G rows per wave, every
// table's rows as one 64-bit range.  A lane loads E = 16 elements per chunk (VEC: 16-B loads, the codes leave as
// one 16-B store) or one; the row's min / max cross the group by ds_bpermute (__shfl_xor).  Min and max are exact
// in any order, so the codes do not depend on the tree.  A row longer than G * E (D > 1024) keeps its first chunk
// in registers and reads the others again for the codes.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void q8_quantize_kernel(const TableDesc* __restrict__ src,
                                                          const Q8Desc* __restrict__ dst, int ntab, int D, int gshift,
                                                          int64_t rows) {
    constexpr int E = VEC ? 16 : 1;
    const int G = 1 << gshift, RPW = 64 >> gshift;
    const int lane = threadIdx.x & 63;
    const int g = lane >> gshift, v = lane & (G - 1);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r0 = wave * RPW; r0 < rows; r0 += nwaves * RPW) {
        const bool live = r0 + g < rows;
        const int64_t r = live ? r0 + g : rows - 1;  // (a dead group repeats the last row and stores nothing)
        const int t = q8_find_table(dst, ntab, r);
        const Q8Desc de = load_q8(dst, t);
        const int64_t local = r - de.row0;
        const T* srow = (const T*)load_table(src, t).data + local * D;
        uint8_t* qrow = de.q + local * D;
        float lo = INFINITY, hi = -INFINITY;
        float f0[E];
#pragma unroll
        for (int e = 0; e < E; ++e) f0[e] = 0.0f;
        for (int c0 = v * E, k = 0; c0 < D; c0 += G * E, ++k) {
            float f[E];
            load_row<T, E>(srow, c0, f);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                lo = fminf(lo, f[e]);
                hi = fmaxf(hi, f[e]);
                if (k == 0) f0[e] = f[e];
            }
        }
        for (int m = G >> 1; m > 0; m >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, m));
            hi = fmaxf(hi, __shfl_xor(hi, m));
        }
        const float range = hi - lo;
        const float scale = range / 255.0f;
        const float inv = range > 0.0f ? 255.0f / range : 0.0f;
        if (!live) continue;
        for (int c0 = v * E, k = 0; c0 < D; c0 += G * E, ++k) {
            float f[E];
            if (k == 0) {
#pragma unroll
                for (int e = 0; e < E; ++e) f[e] = f0[e];
            } else {
                load_row<T, E>(srow, c0, f);
            }
            uint32_t code[E];
#pragma unroll
            for (int e = 0; e < E; ++e) code[e] = q8_code(f[e], lo, inv);
            q8_store_codes<E>(qrow + c0, code);
        }
        if (v == 0) stg<float2>(de.sb + local, float2{scale, lo});
    }
}

// ---------------------------------------------------------------------------- dequantizer
// One lane per E codes: v (fp32) or bf16(v) into an existing table set.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void q8_dequantize_kernel(const Q8Desc* __restrict__ src,
                                                            const TableDesc* __restrict__ dst, int ntab, int D,
                                                            int64_t rows) {
    constexpr int E = VEC ? 16 : 1;
    const int cpr = D / E;
    const int64_t total = rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cpr;
        const int c0 = (int)(i - r * cpr) * E;
        const int t = q8_find_table(src, ntab, r);
        const Q8Desc de = load_q8(src, t);
        const int64_t local = r - de.row0;
        const float2 sb = ldg<float2>(de.sb + local);
        float f[E];
        q8_load_codes<E>(de.q + local * D + c0, f);
#pragma unroll
        for (int e = 0; e < E; ++e) f[e] = q8_value(f[e], sb.x, sb.y);
        store_row<T, E>((T*)load_table(dst, t).data + local * D, c0, f);
    }
}

// ---------------------------------------------------------------------------- gather
// dlrm_maplookup on quantized rows, in maplookup_vec's shape: a lane owns E codes of U (sample, table) items; per
// round of KB lookups every index load (with the descriptors) is issued first, then every code load together with
// its row's {scale, bias} load -- both addresses hang on the index alone, so the dequantization waits for the two
// at once and adds no dependent round trip -- then the k-ordered fp32 sums (seeded with the first row) of the rows
// as their consumer holds them (v, or bf16(v)), converted once: dlrm_maplookup over the dequantized set, bit for bit.  An out-of-range index reads the zero row with scale = bias = 0 (a zero row) and raises the flag after the
// stores.
template <typename T, bool VEC, int U, int KB>
__global__ __launch_bounds__(256) void q8_maplookup_kernel(const Q8Desc* __restrict__ tabs, int ntab, int D,
                                                           const void* __restrict__ idx, int itype, int64_t tstride,
                                                           int base, int B, int L, T* __restrict__ out, int64_t out_ld,
                                                           int64_t out_off, unsigned* __restrict__ err) {
    constexpr int E = VEC ? 16 : 1;
    const int cpr = D / E;
    const int64_t total = (int64_t)ntab * B * cpr;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    const uint8_t* zero8 = (const uint8_t*)g_zero_row;
    const float2* zero2 = (const float2*)g_zero_row;
    bool bad = false;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < total; i0 += nthreads * U) {
        bool live[U];
        int c0[U], tt[U];
        int64_t bb[U];
        Q8Desc td[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t item = i0 + u * nthreads;
            live[u] = item < total;
            const int64_t it = live[u] ? item : 0;
            const int64_t bt = it / cpr;
            c0[u] = (int)(it - bt * cpr) * E;
            bb[u] = bt / ntab;
            tt[u] = (int)(bt - bb[u] * ntab);
            td[u] = load_q8(tabs, tt[u]);
        }
        float acc[U][E];
        for (int k0 = 0; k0 < L; k0 += KB) {
            int64_t ri[U][KB];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int kk = 0; kk < KB; ++kk)
                    ri[u][kk] = load_index_if(live[u] && k0 + kk < L, idx, itype, tt[u] * tstride + bb[u] * L + k0 + kk);
            const uint8_t* qp[U][KB];
            const float2* sp[U][KB];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) {
                    const bool use = live[u] && k0 + kk < L;
                    const int64_t r = ri[u][kk] - base;
                    const bool ok = use & (r >= 0) & (r < td[u].nrows);
                    bad |= use & !ok & (c0[u] == 0);
                    qp[u][kk] = ok ? td[u].q + r * D + c0[u] : zero8;
                    sp[u][kk] = ok ? td[u].sb + r : zero2;
                }
            __builtin_amdgcn_sched_barrier(0);
            typedef typename std::conditional<VEC, uint4, uint8_t>::type raw_t;
            raw_t raw[U][KB];
            float2 sb[U][KB];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) {
                    raw[u][kk] = ldg<raw_t>(qp[u][kk]);
                    sb[u][kk] = ldg<float2>(sp[u][kk]);
                }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int kk = 0; kk < KB; ++kk) {
                    if (k0 + kk >= L) break;
#pragma unroll
                    for (int e = 0; e < E; ++e) {
                        uint32_t code;
                        if constexpr (VEC) {
                            const uint32_t w = e < 4 ? raw[u][kk].x : (e < 8 ? raw[u][kk].y : (e < 12 ? raw[u][kk].z : raw[u][kk].w));
                            code = (w >> (8 * (e & 3))) & 0xffu;
                        } else {
                            code = raw[u][kk];
                        }
                        // a bf16 consumer's row is bf16(v), as the dequantized set holds it (fp32: the identity)
                        const float f = to_f32(from_f32<T>(q8_value((float)code, sb[u][kk].x, sb[u][kk].y)));
                        acc[u][e] = (k0 + kk == 0) ? f : acc[u][e] + f;
                    }
                }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!live[u]) continue;
            store_row<T, E>(out + bb[u] * out_ld + out_off + (int64_t)tt[u] * D, c0[u], acc[u]);
        }
    }
    if (bad) raise_index_error(err);
}

// ---------------------------------------------------------------------------- fused forward
// The pointers of up to kQ8ArgTables quantized tables by value (as TabPtrs for the fp32 / bf16 forward): a lane's
// code-row and {scale, bias} addresses wait on its index load alone.
struct Q8Ptrs {
    const uint8_t* q[kQ8ArgTables + 1];
    const float2* sb[kQ8ArgTables + 1];
    int64_t n[kQ8ArgTables + 1];
};

// One-hot lookup + interaction over quantized rows, one wave per sample, four samples per workgroup, no ys.
// Load plan: lane (c, q) of row block I owns row 16 I + c (row 0 = x, rows 1 .. F-1 the tables' rows) and, per
// column step, the PER_LANE consecutive columns step * COLS + q * PER_LANE .. -- as fwd_body_onehot, so every MFMA
// operand holds the value the two-launch route's fragment load holds.  What is in flight is raw bytes: one 4-B
// (fp32: 4 codes) or 8-B (bf16: 8 codes) load per row block and step, a quarter of the fp32 forward's load
// registers, plus each row's {scale, bias} (one 8-B load per row block, issued with the first codes) and x's own
// 16-B fragments, which only the lanes c == 0 of block 0 read (the others read the zero row).  All loads of a
// column block (128 columns at the compiled d = 128, else 64) are issued before its first conversion; a step's
// codes become floats (v_cvt_f32_ubyte0..3), then values (q8_value), then bf16 where T is, just before its MFMAs.
// Sums: even / odd column-step partials in ascending step order, Z = even + odd (fwd_onehot.hpp).
template <typename T, int NB, int DC>
__global__ __launch_bounds__(256, 2) void q8_fwd_kernel(int d_, int F, int B, const T* __restrict__ x, int64_t x_ld,
                                                        T* __restrict__ out, int64_t out_ld, int padding,
                                                        const void* __restrict__ idx, int itype, int64_t tstride,
                                                        int base, unsigned* __restrict__ err, Q8Ptrs tp) {
    __shared__ __attribute__((aligned(16))) float stage_all[4 * kStage];
    typedef Frag<T> FR;
    typedef typename FR::type frag;
    constexpr int PL = FR::PER_LANE;
    typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
    typedef typename std::conditional<PL == 4, uint32_t, u32x2_t>::type raw_t;
    constexpr int NT = NB * (NB + 1) / 2;
    constexpr int UU = (DC > 0 ? 128 : 64) / FR::COLS;  // column steps per block (even: a step's parity is v & 1)
    static_assert(UU % 2 == 0, "parity of a step within its block");
    const int d = DC > 0 ? DC : d_;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int P = F * (F - 1) / 2;
    const int W = d + P + padding;
    const bool staged = W <= kStage;
    float* stage = stage_all + w * kStage;
    const T* zero = (const T*)g_zero_row;
    const uint8_t* zero8 = (const uint8_t*)g_zero_row;
    bool bad_any = false;
    for (int64_t b = (int64_t)blockIdx.x * 4 + w; b < B; b += (int64_t)gridDim.x * 4) {
        const T* xb = x + b * x_ld;
        T* orow = out + b * out_ld;
        // every index load first (one round trip), then the checks and the {scale, bias} loads
        int64_t ri[NB];
#pragma unroll
        for (int I = 0; I < NB; ++I) {
            const int row = I * 16 + c;
            const bool tab = row >= 1 && row < F;
            ri[I] = load_index_if(tab, idx, itype, tab ? (row - 1) * tstride + b : 0);
        }
        const uint8_t* src[NB];  // the code row, or null: row 0 (x), a padding row, an index out of range
        float2 sb[NB];
#pragma unroll
        for (int I = 0; I < NB; ++I) {
            const int row = I * 16 + c;
            const bool tab = row >= 1 && row < F;
            const int t = tab ? row - 1 : 0;
            const int64_t r = ri[I] - base;
            const bool ok = tab & (r >= 0) & (r < tp.n[t]);
            bad_any |= tab & !ok & (q == 0);
            src[I] = ok ? tp.q[t] + r * d : nullptr;
            sb[I] = ldg<float2>(ok ? tp.sb[t] + r : (const float2*)g_zero_row);
        }
        f32x4_t acc[2][NT];
#pragma unroll
        for (int pp = 0; pp < 2; ++pp)
#pragma unroll
            for (int k = 0; k < NT; ++k) acc[pp][k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        for (int u0 = 0; u0 < d; u0 += UU * FR::COLS) {
            __builtin_amdgcn_sched_barrier(0);
            raw_t raw[UU][NB];
            frag xf[UU];
#pragma unroll
            for (int v = 0; v < UU; ++v) {
                const int col = u0 + v * FR::COLS + q * PL;
                // column steps wholly past d (wave-uniform) issue no load
                if (DC > 0 ? (v * FR::COLS < DC) : (u0 + v * FR::COLS < d)) {
                    const bool in = col < d;
#pragma unroll
                    for (int I = 0; I < NB; ++I) raw[v][I] = ldg<raw_t>((src[I] && in) ? src[I] + col : zero8);
                    xf[v] = ldg<frag>((c == 0 && in) ? xb + col : zero);
                } else {
#pragma unroll
                    for (int I = 0; I < NB; ++I) raw[v][I] = raw_t{};
                    xf[v] = FR::zero();
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int v = 0; v < UU; ++v) {
                if (!(DC > 0 ? (v * FR::COLS < DC) : (u0 + v * FR::COLS < d))) continue;  // (wave-uniform)
                const int col = u0 + v * FR::COLS + q * PL;
                const bool in = col < d;
                frag a[NB];
#pragma unroll
                for (int I = 0; I < NB; ++I) {
                    // a lane past d, a padding row and an out-of-range index are zero rows: scale = bias = 0
                    const bool use = src[I] && in;
                    const float s = use ? sb[I].x : 0.0f, bi = use ? sb[I].y : 0.0f;
                    float f[PL];
#pragma unroll
                    for (int k = 0; k < PL; ++k) {
                        uint32_t word;
                        if constexpr (PL == 4) word = raw[v][I];
                        else word = raw[v][I][k >> 2];
                        f[k] = q8_value((float)((word >> (8 * (k & 3))) & 0xffu), s, bi);
                    }
                    a[I] = FR::from_f(f);
                }
                if (c == 0) a[0] = xf[v];  // row 0 is x, unquantized
                int ij = 0;
#pragma unroll
                for (int I = 0; I < NB; ++I)
#pragma unroll
                    for (int J = 0; J <= I; ++J, ++ij) FR::mma(acc[v & 1][ij], a[I], a[J]);
                // fast_vcat: x into the output head, from its fragments
                if (c == 0 && in) {
                    float f[PL];
                    FR::to_f(f, xf[v]);
                    if (staged) {
#pragma unroll
                        for (int k = 0; k < PL; k += 4) *(f32x4_t*)(stage + col + k) = f32x4_t{f[k], f[k + 1], f[k + 2], f[k + 3]};
                    } else {
#pragma unroll
                        for (int k = 0; k < PL; ++k) stg<T>(orow + col + k, from_f32<T>(f[k]));
                    }
                }
            }
        }
        // Z = even + odd partials; Z[i][j], i > j, in triangular_slice_kernel! order (i-major) after x
        int ij = 0;
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int J = 0; J <= I; ++J, ++ij) {
                const f32x4_t z = acc[0][ij] + acc[1][ij];
                const int j = J * 16 + c;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = I * 16 + 4 * q + r;
                    if (i < F && j < i) {
                        const int e = d + i * (i - 1) / 2 + j;
                        if (staged) stage[e] = z[r];
                        else stg<T>(orow + e, from_f32<T>(z[r]));
                    }
                }
            }
        for (int e = d + P + lane; e < W; e += 64) {
            if (staged) stage[e] = 0.0f;
            else stg<T>(orow + e, from_f32<T>(0.0f));
        }
        if (staged) {
            wave_lds_sync();
            if constexpr (sizeof(T) == 4 && DC >= 128) {
                store_staged<T, 64>(orow, stage, 0, W, lane);
            } else {
                for (int e = lane; e < W; e += 64) stg<T>(orow + e, from_f32<T>(stage[e]));
            }
            wave_lds_sync();
        }
    }
    if (bad_any) raise_index_error(err);
}

// ---------------------------------------------------------------------------- launchers
static unsigned q8_grid(int64_t items, int per_block, int cus, int per_cu) {
    int64_t g = (items + per_block - 1) / per_block;
    const int64_t cap = (int64_t)cus * per_cu;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

int launch_q8_quantize(dlrm_ctx* ctx, const TableDesc* src, int dtype, bool src16, const Q8Desc* dst, int q_align, int T_,
                       int D, int64_t rows) {
    if (T_ == 0 || rows == 0) return DLRM_OK;
    hipStream_t s = ctx_stream(ctx);
    const bool vec = q8_rows_vec(D, q_align, src16);
    // lanes per row: the smallest power of two that covers the row in one chunk per lane, a wave at the most
    const int chunks = vec ? D / 16 : D;
    int gshift = 0;
    while (gshift < 6 && (1 << gshift) < chunks) ++gshift;
    const int rpw = 64 >> gshift;
    // a streaming kernel: 32 blocks of 4 waves per CU (8 waves per SIMD) cover the HBM latency, the rest grid-strides
    const dim3 grid(q8_grid((rows + rpw - 1) / rpw, 4, ctx_num_cus(ctx), 32)), block(256);
#define DLRM_Q8_GO(T, V) hipLaunchKernelGGL((q8_quantize_kernel<T, V>), grid, block, 0, s, src, dst, T_, D, gshift, rows)
    if (dtype == DLRM_F32) { if (vec) DLRM_Q8_GO(float, true); else DLRM_Q8_GO(float, false); }
    else { if (vec) DLRM_Q8_GO(uint16_t, true); else DLRM_Q8_GO(uint16_t, false); }
#undef DLRM_Q8_GO
    return ctx_hip(ctx, hipGetLastError(), "q8_quantize launch");
}

int launch_q8_dequantize(dlrm_ctx* ctx, const Q8Desc* src, int q_align, const TableDesc* dst, int dtype, bool dst16,
                         int T_, int D, int64_t rows) {
    if (T_ == 0 || rows == 0) return DLRM_OK;
    hipStream_t s = ctx_stream(ctx);
    const bool vec = q8_rows_vec(D, q_align, dst16);
    const dim3 grid(q8_grid(rows * (vec ? D / 16 : D), 256, ctx_num_cus(ctx), 32)), block(256);
#define DLRM_Q8_GO(T, V) hipLaunchKernelGGL((q8_dequantize_kernel<T, V>), grid, block, 0, s, src, dst, T_, D, rows)
    if (dtype == DLRM_F32) { if (vec) DLRM_Q8_GO(float, true); else DLRM_Q8_GO(float, false); }
    else { if (vec) DLRM_Q8_GO(uint16_t, true); else DLRM_Q8_GO(uint16_t, false); }
#undef DLRM_Q8_GO
    return ctx_hip(ctx, hipGetLastError(), "q8_dequantize launch");
}

int launch_q8_maplookup(dlrm_ctx* ctx, const Q8Desc* tabs, int q_align, int T_, int D, const void* idx, int itype,
                        int64_t tstride, int base, int B, int L, int dtype, void* out, int64_t out_ld, int64_t out_off) {
    if (T_ == 0 || B == 0) return DLRM_OK;
    hipStream_t s = ctx_stream(ctx);
    const bool vec = q8_rows_vec(D, q_align, q8_out_rows16(dtype, out, out_ld, out_off));
    const int64_t items = (int64_t)T_ * B * (vec ? D / 16 : D);
    // one-hot: 4 items per lane in flight; pooled: 2 bags x 4 lookups
    const int U = L > 1 ? 2 : 4;
    const dim3 grid(q8_grid((items + U - 1) / U, 256, ctx_num_cus(ctx), 16)), block(256);
    unsigned* err = ctx_error_word(ctx);
#define DLRM_Q8_GO(T, V, U_, KB_)                                                                                       \
    hipLaunchKernelGGL((q8_maplookup_kernel<T, V, U_, KB_>), grid, block, 0, s, tabs, T_, D, idx, itype, tstride, base, B, \
                       L, (T*)out, out_ld, out_off, err)
#define DLRM_Q8_L(T, V) do { if (L > 1) DLRM_Q8_GO(T, V, 2, 4); else DLRM_Q8_GO(T, V, 4, 1); } while (0)
    if (dtype == DLRM_F32) { if (vec) DLRM_Q8_L(float, true); else DLRM_Q8_L(float, false); }
    else { if (vec) DLRM_Q8_L(uint16_t, true); else DLRM_Q8_L(uint16_t, false); }
#undef DLRM_Q8_L
#undef DLRM_Q8_GO
    return ctx_hip(ctx, hipGetLastError(), "q8_maplookup launch");
}

template <typename T>
static void launch_q8_fwd(hipStream_t s, unsigned grid, int NB, int d, int F, int B, const void* x, int64_t x_ld,
                          void* out, int64_t out_ld, int padding, const void* idx, int itype, int64_t tstride, int base,
                          unsigned* err, const Q8Ptrs& tp) {
#define DLRM_Q8_GO(NB_, DC_)                                                                                       \
    hipLaunchKernelGGL((q8_fwd_kernel<T, NB_, DC_>), dim3(grid), dim3(256), 0, s, d, F, B, (const T*)x, x_ld, (T*)out, \
                       out_ld, padding, idx, itype, tstride, base, err, tp)
    if (NB == 1) { if (d == 128) DLRM_Q8_GO(1, 128); else DLRM_Q8_GO(1, 0); }
    else { if (d == 128) DLRM_Q8_GO(2, 128); else DLRM_Q8_GO(2, 0); }
#undef DLRM_Q8_GO
}

int launch_q8_lookup_interact_fwd(dlrm_ctx* ctx, const Q8Desc* htabs, int q_align, int T_, int d, const void* idx,
                                  int itype, int64_t tstride, int base, int B, int L, int dtype, const void* x,
                                  int64_t x_ld, void* out, int64_t out_ld, int padding) {
    if (!q8_fwd_fused(dtype, d, T_, L, q_align, x, x_ld)) return DLRM_E_UNSUPPORTED;
    if (B == 0) return DLRM_OK;
    Q8Ptrs tp{};
    for (int t = 0; t < T_; ++t) {
        tp.q[t] = htabs[t].q;
        tp.sb[t] = htabs[t].sb;
        tp.n[t] = htabs[t].nrows;
    }
    const int F = T_ + 1, NB = (F + 15) / 16;
    const unsigned grid = q8_grid(B, 4, ctx_num_cus(ctx), 16);
    if (dtype == DLRM_F32)
        launch_q8_fwd<float>(ctx_stream(ctx), grid, NB, d, F, B, x, x_ld, out, out_ld, padding, idx, itype, tstride, base,
                             ctx_error_word(ctx), tp);
    else
        launch_q8_fwd<uint16_t>(ctx_stream(ctx), grid, NB, d, F, B, x, x_ld, out, out_ld, padding, idx, itype, tstride,
                                base, ctx_error_word(ctx), tp);
    return ctx_hip(ctx, hipGetLastError(), "q8_lookup_interact_fwd launch");
}

}  // namespace dlrm
