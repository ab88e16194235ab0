// q4.hip — int4 row-quantized embedding tables with in-row scale and bias, for inference and evaluation on gfx950.
//
// Format (include/dlrm_hip.h): table t is ONE caller-owned byte array r[N_t][S],
// S = 8 + 8 * ceil(D / 16), every row 8-B aligned: float scale, float bias, then code c in byte 8 + c / 2 (low nibble
// for even c), pad nibbles and bytes zero.  Per row w[0..D), every operation a separately rounded fp32 operation:
//   lo = min w, hi = max w, range = hi - lo, scale = range / 15, inv = range > 0 ? 15 / range : 0
//   q[c] = min(15, max(0, rint((w[c] - lo) * inv)))   (ties to even),   bias = lo
//   v[c] = (q[c] * scale) + bias                       (two roundings, never an fma: q4_value)
// A bf16 consumer gets f32_to_bf16(v[c]).  An all-zero row is a zero row: what an index out of range reads.
//
// Kernels: the quantizer (one lane group per row, a lane per 16 elements = one 8-byte piece of codes), the
// dequantizer (the way back, and every test's yardstick), the dequantizing gather (dlrm_maplookup on quantized rows)
// and the fused one-hot lookup + interaction forward, which writes the bits that the gather + interact.hip's forward
// write: the same MFMA lane layout (fwd_onehot.hpp: lane (c, q) holds columns step * COLS + q * PER_LANE .. of row
// 16 I + c) and the same even / odd column-step partials.  Its loads are wide: the four lanes that own a row fetch
// 16 bytes of it each and bring the nibbles into operand order by a 4 x 4 dword transpose in registers
// (v_permlane32_swap, v_permlane16_swap).  The pooled forward (q4_bags_fwd_kernel) serves bags of
// any size and up to 95 tables with the same bits: a workgroup per sample pools the bags into an LDS operand tile in the
// gather's rounds and runs the Gram from it.
#include <type_traits>

#include "fwd_onehot.hpp"
#include "q4.hpp"

namespace dlrm {

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
// 16 bytes of a row: rows are 8-B aligned, and so is every piece of one
typedef u32x4_t u32x4_a8_t __attribute__((aligned(8)));
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ u32x4_t q4_ldg16(const uint8_t* p) { return *(const DLRM_GLOBAL u32x4_a8_t*)p; }
#else  // host pass of the device code: never executed
__device__ __forceinline__ u32x4_t q4_ldg16(const uint8_t* p) { return *(const u32x4_a8_t*)p; }
#endif

// q * scale + bias in two roundings: q8.hip's q8_value.  The library is built with -ffp-contract=fast, which fuses
// a multiply into a dependent add whatever a pragma says; the empty asm makes the product a value the combiner
// cannot look through (no instruction is emitted for it).
__device__ __forceinline__ float q4_value(float code, float scale, float bias) {
    float p = code * scale;
    asm("" : "+v"(p));
    return p + bias;
}

__device__ __forceinline__ uint32_t q4_code(float w, float lo, float inv) {
    return (uint32_t)fminf(15.0f, fmaxf(0.0f, rintf((w - lo) * inv)));
}

// A row's header {scale, bias}, read and written as two dwords (a HIP float2 goes through a generic reference, and
// the access comes out as a flat_ instruction)
__device__ __forceinline__ float2 q4_load_header(const uint8_t* row) {
    const u32x2_t h = ldg<u32x2_t>(row);
    return float2{__uint_as_float(h[0]), __uint_as_float(h[1])};
}

// nibble k (0 .. 15) of an 8-byte piece of codes, as a float
__device__ __forceinline__ float q4_nibble(const u32x2_t& w, int k) { return (float)((w[k >> 3] >> (4 * (k & 7))) & 15u); }

__device__ __forceinline__ Q4Desc load_q4(const Q4Desc* tabs, int t) {
    const uint4 a = ldg<uint4>(tabs + t);
    const uint2 b = ldg<uint2>((const uint4*)(tabs + t) + 1);
    Q4Desc d;
    d.r = (uint8_t*)(((uint64_t)a.y << 32) | a.x);
    d.nrows = (int64_t)(((uint64_t)a.w << 32) | a.z);
    d.row0 = (int64_t)(((uint64_t)b.y << 32) | b.x);
    d.pad_ = 0;
    return d;
}

// The table that holds row r of the concatenated row range: the last t with row0[t] <= r (empty tables share
// their successor's row0 and are passed over).
__device__ __forceinline__ int q4_find_table(const Q4Desc* tabs, int ntab, int64_t r) {
    int lo = 0, hi = ntab;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ldg<int64_t>(&tabs[mid].row0) <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// 16 consecutive elements of a source / destination row: VEC as 16-B vectors (D % 16 == 0, rows 16-B aligned), else
// one by one, those at or past D left alone
template <typename T, bool VEC> __device__ __forceinline__ void q4_load_elems(const T* row, int c0, int D, float* f) {
    if constexpr (VEC) {
        load_row<T, 16>(row, c0, f);
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) f[e] = c0 + e < D ? to_f32(ldg<T>(row + c0 + e)) : 0.0f;
    }
}
template <typename T, bool VEC> __device__ __forceinline__ void q4_store_elems(T* row, int c0, int D, const float* f) {
    if constexpr (VEC) {
        store_row<T, 16>(row, c0, f);
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (c0 + e < D) stg<T>(row + c0 + e, from_f32<T>(f[e]));
    }
}

// ---------------------------------------------------------------------------- quantizer
// One group of G lanes (a power of two, G * 16 >= D where that fits a wave) per row, 64 / G rows per wave, every
// table's rows as one 64-bit range.  A lane owns 16 consecutive elements per chunk: their codes are one 8-byte piece
// of the row and leave as one 8-byte store (pad nibbles zero), lane 0 of the group writes the 8-byte header.  The
// row's min / max cross the group by ds_bpermute (__shfl_xor); min and max are exact in any order, so the codes do
// not depend on the tree.  A row longer than G * 16 (D > 1024) keeps its first chunk in registers and reads the
// others again for the codes.  VEC: how the source row is read (q4_load_elems).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void q4_quantize_kernel(const TableDesc* __restrict__ src,
                                                          const Q4Desc* __restrict__ dst, int ntab, int D, int64_t S,
                                                          int gshift, int64_t rows) {
    const int G = 1 << gshift, RPW = 64 >> gshift;
    const int lane = threadIdx.x & 63;
    const int g = lane >> gshift, v = lane & (G - 1);
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r0 = wave * RPW; r0 < rows; r0 += nwaves * RPW) {
        const bool live = r0 + g < rows;
        const int64_t r = live ? r0 + g : rows - 1;  // (a dead group repeats the last row and stores nothing)
        const int t = q4_find_table(dst, ntab, r);
        const Q4Desc de = load_q4(dst, t);
        const int64_t local = r - de.row0;
        const T* srow = (const T*)load_table(src, t).data + local * D;
        uint8_t* qrow = de.r + local * S;
        float lo = INFINITY, hi = -INFINITY;
        float f0[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) f0[e] = 0.0f;
        for (int c0 = v * 16, k = 0; c0 < D; c0 += G * 16, ++k) {
            float f[16];
            q4_load_elems<T, VEC>(srow, c0, D, f);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (VEC || c0 + e < D) {
                    lo = fminf(lo, f[e]);
                    hi = fmaxf(hi, f[e]);
                }
                if (k == 0) f0[e] = f[e];
            }
        }
        for (int m = G >> 1; m > 0; m >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, m));
            hi = fmaxf(hi, __shfl_xor(hi, m));
        }
        const float range = hi - lo;
        const float scale = range / 15.0f;
        const float inv = range > 0.0f ? 15.0f / range : 0.0f;
        if (!live) continue;
        for (int c0 = v * 16, k = 0; c0 < D; c0 += G * 16, ++k) {
            float f[16];
            if (k == 0) {
#pragma unroll
                for (int e = 0; e < 16; ++e) f[e] = f0[e];
            } else {
                q4_load_elems<T, VEC>(srow, c0, D, f);
            }
            u32x2_t w = {0u, 0u};
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t code = (VEC || c0 + e < D) ? q4_code(f[e], lo, inv) : 0u;
                w[e >> 3] |= code << (4 * (e & 7));
            }
            stg<u32x2_t>(qrow + 8 + (c0 >> 1), w);
        }
        if (v == 0) stg<u32x2_t>(qrow, u32x2_t{__float_as_uint(scale), __float_as_uint(lo)});
    }
}

// ---------------------------------------------------------------------------- dequantizer
// One lane per 8-byte piece of codes: v (fp32) or bf16(v) into an existing table set.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void q4_dequantize_kernel(const Q4Desc* __restrict__ src,
                                                            const TableDesc* __restrict__ dst, int ntab, int D,
                                                            int64_t S, int64_t rows) {
    const int cpr = (D + 15) >> 4;
    const int64_t total = rows * cpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / cpr;
        const int c0 = (int)(i - r * cpr) * 16;
        const int t = q4_find_table(src, ntab, r);
        const Q4Desc de = load_q4(src, t);
        const int64_t local = r - de.row0;
        const uint8_t* row = de.r + local * S;
        const float2 sb = q4_load_header(row);
        const u32x2_t w = ldg<u32x2_t>(row + 8 + (c0 >> 1));
        float f[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) f[e] = q4_value(q4_nibble(w, e), sb.x, sb.y);
        q4_store_elems<T, VEC>((T*)load_table(dst, t).data + local * D, c0, D, f);
    }
}

// ---------------------------------------------------------------------------- pooling round
// One round of KB lookups, k0 .. k0 + KB - 1, of a lane's U (table, sample) items, shared by the gather and the
// pooled fused forward.  Item u is the 8-byte piece (16 codes) at column c0[u] of table td[u]'s bag whose first index
// sits at position ip[u]; a dead item (live[u] false) reads the zero row and sums to zero.  Every index load is issued
// first, then every piece load together with its row's header load -- the first 8 bytes of the same row, one address
// computation off the index and as a rule the same 128-B line, not a second array -- then the k-ordered fp32 sums
// (seeded with the first row) of the rows as their consumer holds them (v, or bf16(v)).  An out-of-range index reads
// 16 bytes of the zero row (scale = bias = 0: a zero row) and sets bad in the lane that owns the row's first piece.
template <typename T, int U, int KB>
__device__ __forceinline__ void q4_pool_round(const Q4Desc* td, const bool* live, const int* c0, const int64_t* ip,
                                              int k0, int L, int64_t S, const void* __restrict__ idx, int itype, int base,
                                              float (*acc)[16], bool& bad) {
    const uint8_t* zero8 = (const uint8_t*)g_zero_row;
    int64_t ri[U][KB];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) ri[u][kk] = load_index_if(live[u] && k0 + kk < L, idx, itype, ip[u] + k0 + kk);
    const uint8_t* hp[U][KB];  // the row (its header), and this lane's piece of it
    const uint8_t* pp[U][KB];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) {
            const bool use = live[u] && k0 + kk < L;
            const int64_t r = ri[u][kk] - base;
            const bool ok = use & (r >= 0) & (r < td[u].nrows);
            bad |= use & !ok & (c0[u] == 0);
            hp[u][kk] = ok ? td[u].r + r * S : zero8;
            pp[u][kk] = ok ? td[u].r + r * S + 8 + (c0[u] >> 1) : zero8 + 8;
        }
    __builtin_amdgcn_sched_barrier(0);
    u32x2_t raw[U][KB];
    float2 sb[U][KB];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) {
            raw[u][kk] = ldg<u32x2_t>(pp[u][kk]);
            sb[u][kk] = q4_load_header(hp[u][kk]);
        }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) {
            if (k0 + kk >= L) break;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                // a bf16 consumer's row is bf16(v), as the dequantized set holds it (fp32: the identity)
                const float f = to_f32(from_f32<T>(q4_value(q4_nibble(raw[u][kk], e), sb[u][kk].x, sb[u][kk].y)));
                acc[u][e] = (k0 + kk == 0) ? f : acc[u][e] + f;
            }
        }
}

// ---------------------------------------------------------------------------- gather
// dlrm_maplookup on quantized rows, in q8_maplookup_kernel's round structure: a lane owns one 8-byte piece (16 codes)
// of U (sample, table) items and sums it over the bag in rounds of KB lookups (q4_pool_round), converted once:
// dlrm_maplookup over the dequantized set, bit for bit.  The bounds flag is raised after the stores.  VEC: how the
// output row is written (q4_store_elems).
template <typename T, bool VEC, int U, int KB>
__global__ __launch_bounds__(256) void q4_maplookup_kernel(const Q4Desc* __restrict__ tabs, int ntab, int D, int64_t S,
                                                           const void* __restrict__ idx, int itype, int64_t tstride,
                                                           int base, int B, int L, T* __restrict__ out, int64_t out_ld,
                                                           int64_t out_off, unsigned* __restrict__ err) {
    const int cpr = (D + 15) >> 4;
    const int64_t total = (int64_t)ntab * B * cpr;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    bool bad = false;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < total; i0 += nthreads * U) {
        bool live[U];
        int c0[U], tt[U];
        int64_t bb[U];
        Q4Desc td[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t item = i0 + u * nthreads;
            live[u] = item < total;
            const int64_t it = live[u] ? item : 0;
            const int64_t bt = it / cpr;
            c0[u] = (int)(it - bt * cpr) * 16;
            bb[u] = bt / ntab;
            tt[u] = (int)(bt - bb[u] * ntab);
            td[u] = load_q4(tabs, tt[u]);
        }
        int64_t ip[U];
#pragma unroll
        for (int u = 0; u < U; ++u) ip[u] = tt[u] * tstride + bb[u] * L;
        float acc[U][16];
        for (int k0 = 0; k0 < L; k0 += KB) q4_pool_round<T, U, KB>(td, live, c0, ip, k0, L, S, idx, itype, base, acc, bad);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!live[u]) continue;
            q4_store_elems<T, VEC>(out + bb[u] * out_ld + out_off + (int64_t)tt[u] * D, c0[u], D, acc[u]);
        }
    }
    if (bad) raise_index_error(err);
}

// ---------------------------------------------------------------------------- fused forward
// The pointers of up to kQ4ArgTables quantized tables by value (as TabPtrs for the fp32 / bf16 forward): a lane's
// row address waits on its index load alone.
struct Q4Ptrs {
    const uint8_t* r[kQ4ArgTables + 1];
    int64_t n[kQ4ArgTables + 1];
};

// A 4 x 4 dword transpose among the four lanes (c, 0 .. 3) = c, c + 16, c + 32, c + 48: in, lane q' holds a[j];
// out, lane q holds a[q'] = what lane q' held in a[q].  Writing q = 2 hi + lo and j = 2 jh + jl, v_permlane32_swap
// exchanges the (hi, jh) bit pair -- it swaps lanes 32 .. 63 of its first operand with lanes 0 .. 31 of its second --
// and v_permlane16_swap the (lo, jl) pair (the odd 16-lane rows of the first with the even rows of the second).
// Four instructions, no LDS.  Every lane of the wave takes part (the callers are wave-uniform).
__device__ __forceinline__ void q4_transpose4(uint32_t* a) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int jl = 0; jl < 2; ++jl) {
        const u32x2_t s = __builtin_amdgcn_permlane32_swap(a[jl], a[2 + jl], false, false);
        a[jl] = s[0];
        a[2 + jl] = s[1];
    }
#pragma unroll
    for (int jh = 0; jh < 2; ++jh) {
        const u32x2_t s = __builtin_amdgcn_permlane16_swap(a[2 * jh], a[2 * jh + 1], false, false);
        a[2 * jh] = s[0];
        a[2 * jh + 1] = s[1];
    }
#endif
}

// One-hot lookup + interaction over quantized rows, one wave per sample, four samples per workgroup, no ys.
// Operand layout: lane (c, q) of row block I owns row 16 I + c (row 0 = x, rows 1 .. F-1 the tables' rows) and, per
// column step, the PER_LANE consecutive columns step * COLS + q * PER_LANE .. -- as fwd_body_onehot, so every MFMA
// operand holds the value the two-launch route's fragment load holds.
// Load plan, per block of 128 columns = 64 bytes of codes: lane (c, q) fetches bytes 16 q .. 16 q + 15 of them, its
// dwords p[0 .. 3], in one 16-byte load (the compiled d = 128; rows are 8-B aligned, and so is the load) or two
// 8-byte loads (any other d: a piece past the row's end reads the zero row instead), and the row's header, its first
// 8 bytes, in the same round: two wave-instructions per row block cover a d = 128 row where the int8 forward issues
// eight (fp32) or four (bf16) plus one.  Every load of the block, x's 16-B fragments included (which only the lanes
// c == 0 of block 0 read; the others read the zero row), is issued before the first conversion: at d <= 128 that is
// all of a sample's rows.
// Into operand order, in registers:
//   bf16: at step v lane (c, q) needs the 8 codes of columns 32 v + 8 q .., dword 4 v + q of the block: what lane
//         (c, v) holds in p[q].  q4_transpose4.
//   fp32: at step v lane (c, q) needs the 4 codes of columns 16 v + 4 q .., the 2-byte unit 4 v + q; lane (c, q')
//         holds units 8 q' .. 8 q' + 7.  It first pairs the two units each reader wants from it, w[q] = {unit q, unit
//         4 + q} (a byte select per dword), then the same transpose: lane (c, q) ends with w[q'] = the units of steps
//         2 q' (low half) and 2 q' + 1 (high half).
// Unpacking: even = w & 0x0f0f0f0f and odd = (w >> 4) & 0x0f0f0f0f hold one code per byte; v_cvt_f32_ubyte0..3, then
// q4_value, then bf16 where T is, just before the step's MFMAs.
// Sums: even / odd column-step partials in ascending step order, Z = even + odd (fwd_onehot.hpp).
template <typename T, int NB, int DC>
__global__ __launch_bounds__(256, 2) void q4_fwd_kernel(int d_, int F, int B, const T* __restrict__ x, int64_t x_ld,
                                                        T* __restrict__ out, int64_t out_ld, int padding,
                                                        const void* __restrict__ idx, int itype, int64_t tstride,
                                                        int base, unsigned* __restrict__ err, Q4Ptrs tp) {
    __shared__ __attribute__((aligned(16))) float stage_all[4 * kStage];
    typedef Frag<T> FR;
    typedef typename FR::type frag;
    constexpr int PL = FR::PER_LANE;
    constexpr int NT = NB * (NB + 1) / 2;
    constexpr int UU = 128 / FR::COLS;  // column steps per block (even: a step's parity is v & 1)
    static_assert(UU % 2 == 0, "parity of a step within its block");
    const int d = DC > 0 ? DC : d_;
    const int64_t S = 8 + (d >> 1);  // (d % 16 == 0: q4_row_bytes)
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
        // every index load first (one round trip), then the checks and the header loads
        int64_t ri[NB];
#pragma unroll
        for (int I = 0; I < NB; ++I) {
            const int row = I * 16 + c;
            const bool tab = row >= 1 && row < F;
            ri[I] = load_index_if(tab, idx, itype, tab ? (row - 1) * tstride + b : 0);
        }
        const uint8_t* src[NB];  // the row, or null: row 0 (x), a padding row, an index out of range
        float2 sb[NB];
#pragma unroll
        for (int I = 0; I < NB; ++I) {
            const int row = I * 16 + c;
            const bool tab = row >= 1 && row < F;
            const int t = tab ? row - 1 : 0;
            const int64_t r = ri[I] - base;
            const bool ok = tab & (r >= 0) & (r < tp.n[t]);
            bad_any |= tab & !ok & (q == 0);
            src[I] = ok ? tp.r[t] + r * S : nullptr;
            sb[I] = q4_load_header(ok ? src[I] : zero8);
        }
        f32x4_t acc[2][NT];
#pragma unroll
        for (int pp = 0; pp < 2; ++pp)
#pragma unroll
            for (int k = 0; k < NT; ++k) acc[pp][k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        for (int u0 = 0; u0 < d; u0 += 128) {
            __builtin_amdgcn_sched_barrier(0);
            uint32_t p[NB][4];
            frag xf[UU];
            const int pb = (u0 >> 1) + 16 * q;  // this lane's piece: byte pb of the codes ...
            const int rem = (d >> 1) - pb;      // ... of which rem (a multiple of 8) are left at and after it
#pragma unroll
            for (int I = 0; I < NB; ++I) {
                if constexpr (DC == 128) {
                    const u32x4_t v4 = q4_ldg16(src[I] ? src[I] + 8 + 16 * q : zero8);
                    p[I][0] = v4[0]; p[I][1] = v4[1]; p[I][2] = v4[2]; p[I][3] = v4[3];
                } else {
                    const u32x2_t l2 = ldg<u32x2_t>((src[I] && rem >= 8) ? src[I] + 8 + pb : zero8);
                    const u32x2_t h2 = ldg<u32x2_t>((src[I] && rem >= 16) ? src[I] + 16 + pb : zero8);
                    p[I][0] = l2[0]; p[I][1] = l2[1]; p[I][2] = h2[0]; p[I][3] = h2[1];
                }
            }
#pragma unroll
            for (int v = 0; v < UU; ++v) {
                const int col = u0 + v * FR::COLS + q * PL;
                // column steps wholly past d (wave-uniform) issue no load
                if (DC > 0 ? (v * FR::COLS < DC) : (u0 + v * FR::COLS < d)) xf[v] = ldg<frag>((c == 0 && col < d) ? xb + col : zero);
                else xf[v] = FR::zero();
            }
            __builtin_amdgcn_sched_barrier(0);
            // the codes into operand order, then one code per byte: ev the even codes of a dword, od the odd ones (the
            // empty asm keeps the byte lanes whole, so that each code is one v_cvt_f32_ubyte0..3 away)
            uint32_t ev[NB][4], od[NB][4];
#pragma unroll
            for (int I = 0; I < NB; ++I) {
                if constexpr (PL == 4) {
                    const uint32_t p0 = p[I][0], p1 = p[I][1], p2 = p[I][2], p3 = p[I][3];
                    p[I][0] = (p0 & 0xffffu) | (p2 << 16);
                    p[I][1] = (p0 >> 16) | (p2 & 0xffff0000u);
                    p[I][2] = (p1 & 0xffffu) | (p3 << 16);
                    p[I][3] = (p1 >> 16) | (p3 & 0xffff0000u);
                }
                q4_transpose4(p[I]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ev[I][j] = p[I][j] & 0x0f0f0f0fu;
                    od[I][j] = (p[I][j] >> 4) & 0x0f0f0f0fu;
                    asm("" : "+v"(ev[I][j]), "+v"(od[I][j]));
                }
            }
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
                    // fp32: the step's 4 codes are a half of dword v / 2; bf16: its 8 codes are dword v
                    const int j = PL == 4 ? v >> 1 : v, sh = PL == 4 ? 16 * (v & 1) : 0;
                    float f[PL];
#pragma unroll
                    for (int k = 0; k < PL; k += 2) {
                        f[k] = q4_value((float)((ev[I][j] >> (sh + 4 * k)) & 0xffu), s, bi);
                        f[k + 1] = q4_value((float)((od[I][j] >> (sh + 4 * k)) & 0xffu), s, bi);
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

// ---------------------------------------------------------------------------- fused forward, pooled bags
// Lookup (bags of L >= 1 rows, summed) + interaction over quantized rows of 1 .. 95 tables, one launch, no ys: the
// bits of q4_maplookup_kernel + interact.hip's forward.  One workgroup of four waves per sample, grid-strided over the
// batch; per column block of CB columns (q4_plan.hpp: the whole d, or 128 at a time) two phases around a barrier.
// Phase A, pool: the block's T x CB / 16 pieces are dealt over the 256 lanes, one to a lane at a time, and summed
//   over the bag by q4_pool_round (the gather's rounds of 4 lookups, its arithmetic and its order); the pooled piece,
//   rounded to T once, goes to row t + 1 of the LDS operand tile rows[16 NB][CB + pad].  Row 0 is x, loaded in 16-B
//   fragments before the gather is issued and also copied to the head of the output row; rows F .. 16 NB - 1 are
//   zeroed once per workgroup.  A piece past d inside the block's last column step (bf16, d % 32 == 16) is a dead
//   item: it pools the zero row and so clears its 16 columns of the tile.
// Phase B, Gram: tile k = I (I + 1) / 2 + J of the NB (NB + 1) / 2 lower-triangle 16 x 16 tiles belongs to wave k % 4.
//   A wave walks the block's column steps in ascending order; lane (c, q) reads columns step * COLS + q * PER_LANE ..
//   of rows 16 I + c and 16 J + c from the tile (fwd_onehot.hpp's operand layout, one 16-B LDS read each) and issues
//   Frag<T>::mma into the tile's accumulator, which lives across column blocks.  NB <= 2: even and odd steps in two
//   partials, Z = even + odd; NB >= 3: one chain -- dlrm_interact_fwd's orders.  (A multi-block CB is 128 columns,
//   an even number of steps, so a step's parity within its block is its parity within the row.)
// Output: Z[i][j], i > j, i-major after x, stored from the accumulators (lanes c = 0 .. 15 write 16 consecutive
// elements), then the padding zeros.  out needs no alignment.
extern __shared__ __attribute__((aligned(16))) unsigned char q4_bags_lds[];

template <typename T, int NB>
__global__ __launch_bounds__(256, NB <= 4 ? 4 : 2) void q4_bags_fwd_kernel(const Q4Desc* __restrict__ tabs, int d, int F, int B, int CB,
                                                             const T* __restrict__ x, int64_t x_ld, T* __restrict__ out,
                                                             int64_t out_ld, int padding, const void* __restrict__ idx,
                                                             int itype, int64_t tstride, int base, int L,
                                                             unsigned* __restrict__ err) {
    typedef Frag<T> FR;
    typedef typename FR::type frag;
    constexpr int PL = FR::PER_LANE, COLS = FR::COLS;  // PL elements = 16 bytes
    constexpr int NT = NB * (NB + 1) / 2, MT = (NT + 3) / 4, NPART = NB <= 2 ? 2 : 1;
    constexpr int U = 1, KB = 4;
    T* rows = (T*)q4_bags_lds;
    const int LD = CB + PL;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, q = lane >> 4;
    const int ntab = F - 1;
    const int64_t S = 8 + (d >> 1);  // (d % 16 == 0: q4_row_bytes)
    const int P = F * (F - 1) / 2, W = d + P + padding;
    const T* zero = (const T*)g_zero_row;
    for (int i = F * (LD / PL) + tid; i < 16 * NB * (LD / PL); i += 256) *(frag*)(rows + i * PL) = FR::zero();
    int tI[MT], tJ[MT];  // this wave's tiles
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int k = w + 4 * m;
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= k) ++I;
        tI[m] = I;
        tJ[m] = k - I * (I + 1) / 2;
    }
    bool bad = false;
    for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
        const T* xb = x + b * x_ld;
        T* orow = out + b * out_ld;
        f32x4_t acc[NPART][MT];
#pragma unroll
        for (int pp = 0; pp < NPART; ++pp)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[pp][m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        for (int u0 = 0; u0 < d; u0 += CB) {
            const int valid = d - u0 < CB ? d - u0 : CB;         // columns of this block inside d ...
            const int vpad = (valid + COLS - 1) / COLS * COLS;  // ... and up to the end of its last column step
            // ---- phase A
            const int xc = tid * PL;
            frag xf = FR::zero();
            if (xc < vpad) xf = ldg<frag>(xc < valid ? xb + u0 + xc : zero);
            const int ppb = vpad >> 4, nitems = ntab * ppb;
            for (int it0 = tid; it0 < nitems; it0 += 256 * U) {
                bool have[U], live[U];
                int c0[U], tt[U];
                int64_t ip[U];
                Q4Desc td[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int item = it0 + 256 * u;
                    have[u] = item < nitems;
                    tt[u] = have[u] ? item / ppb : 0;
                    const int col = (have[u] ? item - tt[u] * ppb : 0) * 16;
                    c0[u] = u0 + col;
                    live[u] = have[u] && col < valid;
                    td[u] = load_q4(tabs, tt[u]);
                    ip[u] = tt[u] * tstride + b * L;
                }
                float sum[U][16];
                for (int k0 = 0; k0 < L; k0 += KB)
                    q4_pool_round<T, U, KB>(td, live, c0, ip, k0, L, S, idx, itype, base, sum, bad);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (!have[u]) continue;
                    T* dst = rows + (tt[u] + 1) * LD + (c0[u] - u0);
#pragma unroll
                    for (int e = 0; e < 16; e += PL) *(frag*)(dst + e) = FR::from_f(sum[u] + e);
                }
            }
            if (xc < vpad) {
                *(frag*)(rows + xc) = xf;
                if (xc < valid) {
                    float f[PL];
                    FR::to_f(f, xf);
#pragma unroll
                    for (int k = 0; k < PL; ++k) stg<T>(orow + u0 + xc + k, from_f32<T>(f[k]));
                }
            }
            __syncthreads();
            // ---- phase B
            const int nsteps = vpad / COLS;
            for (int v = 0; v < nsteps; v += 2) {
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) {
                    if (v + pp >= nsteps) break;
                    const int col = (v + pp) * COLS + q * PL;
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        if (w + 4 * m >= NT) break;  // (wave-uniform)
                        const frag a = *(const frag*)(rows + (16 * tI[m] + c) * LD + col);
                        const frag bj = *(const frag*)(rows + (16 * tJ[m] + c) * LD + col);
                        FR::mma(acc[NPART == 2 ? pp : 0][m], a, bj);
                    }
                }
            }
            __syncthreads();  // the next block, or the next sample, rewrites the tile
        }
        // Z[i][j], i > j: triangular_slice_kernel! order (i-major), after x
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (w + 4 * m >= NT) break;
            const f32x4_t z = NPART == 2 ? acc[0][m] + acc[NPART - 1][m] : acc[0][m];
            const int j = tJ[m] * 16 + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = tI[m] * 16 + 4 * q + r;
                if (i < F && j < i) stg<T>(orow + d + i * (i - 1) / 2 + j, from_f32<T>(z[r]));
            }
        }
        for (int e = d + P + tid; e < W; e += 256) stg<T>(orow + e, from_f32<T>(0.0f));
    }
    if (bad) raise_index_error(err);
}

// ---------------------------------------------------------------------------- launchers
static unsigned q4_grid(int64_t items, int per_block, int cus, int per_cu) {
    int64_t g = (items + per_block - 1) / per_block;
    const int64_t cap = (int64_t)cus * per_cu;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

int launch_q4_quantize(dlrm_ctx* ctx, const TableDesc* src, int dtype, bool src16, const Q4Desc* dst, int T_, int D,
                       int64_t rows) {
    if (T_ == 0 || rows == 0) return DLRM_OK;
    hipStream_t s = ctx_stream(ctx);
    const bool vec = q4_rows_vec(D, src16);
    const int64_t S = q4_row_bytes(D);
    // lanes per row: the smallest power of two that covers the row in one chunk per lane, a wave at the most
    const int chunks = (D + 15) / 16;
    int gshift = 0;
    while (gshift < 6 && (1 << gshift) < chunks) ++gshift;
    const int rpw = 64 >> gshift;
    // a streaming kernel: 32 blocks of 4 waves per CU (8 waves per SIMD) cover the HBM latency, the rest grid-strides
    const dim3 grid(q4_grid((rows + rpw - 1) / rpw, 4, ctx_num_cus(ctx), 32)), block(256);
#define DLRM_Q4_GO(T, V) hipLaunchKernelGGL((q4_quantize_kernel<T, V>), grid, block, 0, s, src, dst, T_, D, S, gshift, rows)
    if (dtype == DLRM_F32) { if (vec) DLRM_Q4_GO(float, true); else DLRM_Q4_GO(float, false); }
    else { if (vec) DLRM_Q4_GO(uint16_t, true); else DLRM_Q4_GO(uint16_t, false); }
#undef DLRM_Q4_GO
    return ctx_hip(ctx, hipGetLastError(), "q4_quantize launch");
}

int launch_q4_dequantize(dlrm_ctx* ctx, const Q4Desc* src, const TableDesc* dst, int dtype, bool dst16, int T_, int D,
                         int64_t rows) {
    if (T_ == 0 || rows == 0) return DLRM_OK;
    hipStream_t s = ctx_stream(ctx);
    const bool vec = q4_rows_vec(D, dst16);
    const int64_t S = q4_row_bytes(D);
    const dim3 grid(q4_grid(rows * ((D + 15) / 16), 256, ctx_num_cus(ctx), 32)), block(256);
#define DLRM_Q4_GO(T, V) hipLaunchKernelGGL((q4_dequantize_kernel<T, V>), grid, block, 0, s, src, dst, T_, D, S, rows)
    if (dtype == DLRM_F32) { if (vec) DLRM_Q4_GO(float, true); else DLRM_Q4_GO(float, false); }
    else { if (vec) DLRM_Q4_GO(uint16_t, true); else DLRM_Q4_GO(uint16_t, false); }
#undef DLRM_Q4_GO
    return ctx_hip(ctx, hipGetLastError(), "q4_dequantize launch");
}

int launch_q4_maplookup(dlrm_ctx* ctx, const Q4Desc* tabs, int T_, int D, const void* idx, int itype, int64_t tstride,
                        int base, int B, int L, int dtype, void* out, int64_t out_ld, int64_t out_off) {
    if (T_ == 0 || B == 0) return DLRM_OK;
    hipStream_t s = ctx_stream(ctx);
    const bool vec = q4_rows_vec(D, q4_out_rows16(dtype, out, out_ld, out_off));
    const int64_t S = q4_row_bytes(D);
    const int64_t items = (int64_t)T_ * B * ((D + 15) / 16);
    // one-hot: 4 items per lane in flight; pooled: 2 bags x 4 lookups
    const int U = L > 1 ? 2 : 4;
    const dim3 grid(q4_grid((items + U - 1) / U, 256, ctx_num_cus(ctx), 16)), block(256);
    unsigned* err = ctx_error_word(ctx);
#define DLRM_Q4_GO(T, V, U_, KB_)                                                                                          \
    hipLaunchKernelGGL((q4_maplookup_kernel<T, V, U_, KB_>), grid, block, 0, s, tabs, T_, D, S, idx, itype, tstride, base, \
                       B, L, (T*)out, out_ld, out_off, err)
#define DLRM_Q4_L(T, V) do { if (L > 1) DLRM_Q4_GO(T, V, 2, 4); else DLRM_Q4_GO(T, V, 4, 1); } while (0)
    if (dtype == DLRM_F32) { if (vec) DLRM_Q4_L(float, true); else DLRM_Q4_L(float, false); }
    else { if (vec) DLRM_Q4_L(uint16_t, true); else DLRM_Q4_L(uint16_t, false); }
#undef DLRM_Q4_L
#undef DLRM_Q4_GO
    return ctx_hip(ctx, hipGetLastError(), "q4_maplookup launch");
}

template <typename T>
static void launch_q4_fwd(hipStream_t s, unsigned grid, int NB, int d, int F, int B, const void* x, int64_t x_ld,
                          void* out, int64_t out_ld, int padding, const void* idx, int itype, int64_t tstride, int base,
                          unsigned* err, const Q4Ptrs& tp) {
#define DLRM_Q4_GO(NB_, DC_)                                                                                       \
    hipLaunchKernelGGL((q4_fwd_kernel<T, NB_, DC_>), dim3(grid), dim3(256), 0, s, d, F, B, (const T*)x, x_ld, (T*)out, \
                       out_ld, padding, idx, itype, tstride, base, err, tp)
    if (NB == 1) { if (d == 128) DLRM_Q4_GO(1, 128); else DLRM_Q4_GO(1, 0); }
    else { if (d == 128) DLRM_Q4_GO(2, 128); else DLRM_Q4_GO(2, 0); }
#undef DLRM_Q4_GO
}

int launch_q4_lookup_interact_fwd(dlrm_ctx* ctx, const Q4Desc* htabs, int T_, int d, const void* idx, int itype,
                                  int64_t tstride, int base, int B, int L, int dtype, const void* x, int64_t x_ld,
                                  void* out, int64_t out_ld, int padding) {
    if (!q4_fwd_fused(dtype, d, T_, L, x, x_ld)) return DLRM_E_UNSUPPORTED;
    if (B == 0) return DLRM_OK;
    Q4Ptrs tp{};
    for (int t = 0; t < T_; ++t) {
        tp.r[t] = htabs[t].r;
        tp.n[t] = htabs[t].nrows;
    }
    const int F = T_ + 1, NB = (F + 15) / 16;
    const unsigned grid = q4_grid(B, 4, ctx_num_cus(ctx), 16);
    if (dtype == DLRM_F32)
        launch_q4_fwd<float>(ctx_stream(ctx), grid, NB, d, F, B, x, x_ld, out, out_ld, padding, idx, itype, tstride, base,
                             ctx_error_word(ctx), tp);
    else
        launch_q4_fwd<uint16_t>(ctx_stream(ctx), grid, NB, d, F, B, x, x_ld, out, out_ld, padding, idx, itype, tstride,
                                base, ctx_error_word(ctx), tp);
    return ctx_hip(ctx, hipGetLastError(), "q4_lookup_interact_fwd launch");
}

template <typename T>
static void launch_q4_bags(hipStream_t s, unsigned grid, unsigned lds, int NB, const Q4Desc* tabs, int d, int F, int B,
                           int CB, const void* x, int64_t x_ld, void* out, int64_t out_ld, int padding, const void* idx,
                           int itype, int64_t tstride, int base, int L, unsigned* err) {
#define DLRM_Q4_GO(NB_)                                                                                               \
    hipLaunchKernelGGL((q4_bags_fwd_kernel<T, NB_>), dim3(grid), dim3(256), lds, s, tabs, d, F, B, CB, (const T*)x, x_ld, \
                       (T*)out, out_ld, padding, idx, itype, tstride, base, L, err)
    switch (NB) {
    case 1: DLRM_Q4_GO(1); break;
    case 2: DLRM_Q4_GO(2); break;
    case 3: DLRM_Q4_GO(3); break;
    case 4: DLRM_Q4_GO(4); break;
    case 5: DLRM_Q4_GO(5); break;
    default: DLRM_Q4_GO(6); break;
    }
#undef DLRM_Q4_GO
}

int launch_q4_bags_interact_fwd(dlrm_ctx* ctx, const Q4Desc* tabs, int T_, int d, const void* idx, int itype,
                                int64_t tstride, int base, int B, int L, int dtype, const void* x, int64_t x_ld, void* out,
                                int64_t out_ld, int padding) {
    if (!q4_bags_fused(dtype, d, T_, L, x, x_ld)) return DLRM_E_UNSUPPORTED;
    if (B == 0) return DLRM_OK;
    const int F = T_ + 1, NB = (F + 15) / 16, CB = q4_bags_cb(dtype, d);
    const unsigned lds = (unsigned)q4_bags_lds_bytes(dtype, d, T_);
    // a workgroup per sample; at most 8 per CU in flight (registers allow 4 at NB <= 4, else 2), the rest grid-strides
    const unsigned grid = q4_grid(B, 1, ctx_num_cus(ctx), 8);
    if (dtype == DLRM_F32)
        launch_q4_bags<float>(ctx_stream(ctx), grid, lds, NB, tabs, d, F, B, CB, x, x_ld, out, out_ld, padding, idx, itype,
                              tstride, base, L, ctx_error_word(ctx));
    else
        launch_q4_bags<uint16_t>(ctx_stream(ctx), grid, lds, NB, tabs, d, F, B, CB, x, x_ld, out, out_ld, padding, idx,
                                 itype, tstride, base, L, ctx_error_word(ctx));
    return ctx_hip(ctx, hipGetLastError(), "q4_bags_interact_fwd launch");
}

}  // namespace dlrm
