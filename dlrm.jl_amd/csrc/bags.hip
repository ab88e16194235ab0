// bags.hip — pooled lookup + interaction forward on fp32 / bf16 tables, one launch, for gfx950.
//
//   ys[b][d + t d + c] = sum_{k < L} table_t[idx_t[b L + k] - base][c]        (only where ys is kept)
//   out[b] = [ x_b | Z[i][j], i = 1 .. F-1, j < i | 0 * padding ],  Z = T_b T_b^T,  T_b = [x_b; the pooled rows]
//
// The bits of dlrm_maplookup(out_offset = d) + dlrm_interact_fwd for bags of any size and 1 .. 95 tables, where the
// forward of interact.hip gives one wave all T L rows of a sample (or, with ys kept, writes ys and reads it back in a
// second launch).  The shape is q4.hip's q4_bags_fwd_kernel -- a workgroup of four waves per sample, the pooled rows
// in an LDS operand tile, the Gram from LDS on MFMA -- on plain rows, with two tiles instead of two barriers.
//
// Work: the unit is (sample, column block of CB columns = bags_cb_bytes); a workgroup walks the units of its samples
// (b = blockIdx.x, + gridDim.x, ..) in sequence, across sample boundaries.  In iteration u every wave does
//   phase A of unit u + 1 into tile (u + 1) & 1, with phase B of unit u from tile u & 1 inside it, then ONE barrier:
// after it tile u & 1 is free for unit u + 2 and tile (u + 1) & 1 is complete.  Iteration -1 has no phase B (the
// prologue) and the last one a phase A of no items.
// Phase A, pool: the block's T x CB / vec items (one 16-B vector of one table's bag) are dealt over the 256 lanes,
//   consecutive lanes on consecutive vectors of a row (32 or 16 lanes read 512 or 256 contiguous bytes of it).  A lane
//   keeps U = 2 items x KB = 4 lookups in flight: every index load of the round, then every row load, unmasked (a dead
//   item or an index out of range reads the zero row), then the sums -- maplookup_vec's pooled round with its
//   arithmetic: seeded with the first row, fp32 adds in lookup order, one rounding by Vec<T>::from_f32, an exact copy
//   at L = 1.  The pooled vector goes to row t + 1 of the tile and, with YS, to ys as a 16-B store.  Row 0 is x, loaded
//   in 16-B fragments before the gather is issued and copied to out[b][0:d] and ys[b][0:d].  A vector past d inside the
//   block's last column step is a dead item: it pools the zero row and clears its columns of the tile.  Rows F ..
//   16 NB - 1 of both tiles are zeroed once per workgroup.
// Phase B, Gram: q4_bags_fwd_kernel's deal and order -- tile k = I (I + 1) / 2 + J of the lower triangle belongs to
//   wave k % 4; lane (c, q) reads columns step * COLS + q * PER_LANE .. of rows 16 I + c and 16 J + c, one 16-B LDS read
//   each, and issues Frag<T>::mma; NB <= 2 keeps even and odd column-step partials and adds them, NB >= 3 one ascending
//   chain: dlrm_interact_fwd's orders.  The accumulators live across a sample's column blocks; the triangle and the
//   padding zeros leave from them at the sample's last block.  It is issued inside phase A's last round, after that
//   round's row loads and before their sums: the MFMAs of unit u run under the outstanding loads of unit u + 1.  A wave
//   without a Gram tile (NB = 1 has one tile, NB = 2 three) goes straight on to its sums.
// The bounds flag is raised after the stores.  No allocation, no memset, no host synchronisation: graph-capturable.
#include "bags.hpp"
#include "fwd_onehot.hpp"

namespace dlrm {

extern __shared__ __attribute__((aligned(16))) unsigned char bags_lds[];

// Workgroups per CU, from the resource report (profiles/bags_fwd/kernels.txt): NB <= 2 needs at most 116 VGPRs (4 waves
// per SIMD), NB = 3 .. 5 at most 160 (3; at NB = 3 and 5 the two tiles allow no more either), NB = 6 192 (2)
constexpr int bags_wg_per_cu(int NB) { return NB <= 2 ? 4 : (NB <= 5 ? 3 : 2); }

template <typename T, int NB, bool YS>
__global__ __launch_bounds__(256, bags_wg_per_cu(NB)) void bags_fwd_kernel(
    const TableDesc* __restrict__ tabs, int d, int F, int B, int CB, const T* __restrict__ x, int64_t x_ld,
    T* __restrict__ ys, int64_t ys_ld, T* __restrict__ out, int64_t out_ld, int padding, const void* __restrict__ idx,
    int itype, int64_t tstride, int base, int L, unsigned* __restrict__ err) {
    typedef Frag<T> FR;
    typedef typename FR::type frag;
    typedef Vec<T> V;
    typedef typename V::type vt;
    constexpr int PL = FR::PER_LANE, COLS = FR::COLS;  // PL elements = 16 bytes = one item
    static_assert(PL == V::N, "an item is one MFMA operand read");
    constexpr int NT = NB * (NB + 1) / 2, MT = (NT + 3) / 4, NPART = NB <= 2 ? 2 : 1;
    constexpr int U = 2, KB = 4;
    const int LD = CB + PL, tile = 16 * NB * LD;
    T* tiles = (T*)bags_lds;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, q = lane >> 4;
    const int ntab = F - 1;
    const int P = F * (F - 1) / 2, W = d + P + padding;
    const vt* zero = (const vt*)g_zero_row;
    for (int i = F * (LD / PL) + tid; i < 16 * NB * (LD / PL); i += 256) {
        *(frag*)(tiles + i * PL) = FR::zero();
        *(frag*)(tiles + tile + i * PL) = FR::zero();
    }
    int tI[MT], tJ[MT];  // this wave's tiles
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const int k = w + 4 * m;
        int I = 0;
        while ((I + 1) * (I + 2) / 2 <= k) ++I;
        tI[m] = I;
        tJ[m] = k - I * (I + 1) / 2;
    }
    f32x4_t acc[NPART][MT];
#pragma unroll
    for (int pp = 0; pp < NPART; ++pp)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[pp][m] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // phase B of one unit: nsteps column steps of the tile rt into the accumulators
    auto gram = [&](const T* rt, int nsteps) {
        for (int v = 0; v < nsteps; v += 2) {
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {
                if (v + pp >= nsteps) break;
                const int col = (v + pp) * COLS + q * PL;
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    if (w + 4 * m >= NT) break;  // (wave-uniform)
                    const frag a = *(const frag*)(rt + (16 * tI[m] + c) * LD + col);
                    const frag bj = *(const frag*)(rt + (16 * tJ[m] + c) * LD + col);
                    FR::mma(acc[NPART == 2 ? pp : 0][m], a, bj);
                }
            }
        }
    };

    const int nblk = (d + CB - 1) / CB;  // column blocks per sample
    const int64_t ns = (int64_t)blockIdx.x < B ? (B - 1 - blockIdx.x) / gridDim.x + 1 : 0;
    const int64_t nunits = ns * nblk;
    int64_t bA = blockIdx.x, bB = blockIdx.x;  // the samples of unit u + 1 (phase A) and of unit u (phase B)
    int kA = 0, kB = 0;                        // ... and their column blocks
    bool bad = false;
    for (int64_t u = -1; u < nunits; ++u) {
        const bool doA = u + 1 < nunits, doB = u >= 0;
        T* wt = tiles + (int)((u + 1) & 1) * tile;
        const T* rt = tiles + (int)(u & 1) * tile;
        // ---- phase A of unit u + 1 (none: no items, one round of dead loads that carries phase B)
        const int u0 = kA * CB;
        const int valid = doA ? (d - u0 < CB ? d - u0 : CB) : 0;  // columns of this block inside d ...
        const int vpad = (valid + COLS - 1) / COLS * COLS;        // ... and up to the end of its last column step
        const T* xb = x + bA * x_ld;
        T* orow = out + bA * out_ld;
        T* yrow = YS ? ys + bA * ys_ld : nullptr;
        const int xc = tid * PL;
        frag xf = FR::zero();
        if (xc < vpad) xf = ldg<frag>(xc < valid ? (const void*)(xb + u0 + xc) : (const void*)zero);
        const int ppb = vpad / PL, nitems = ntab * ppb;
        const int ppb1 = ppb > 0 ? ppb : 1;
        const int Lr = doA ? L : 1;
        // the steps of unit u's block, as its phase A saw them
        const int validB = d - kB * CB < CB ? d - kB * CB : CB;
        const int nstepsB = (validB + COLS - 1) / COLS;
        for (int it0 = 0;; it0 += 256 * U) {
            const bool last_pass = it0 + 256 * U >= nitems;  // (workgroup-uniform)
            bool have[U], live[U];
            int c0[U], tt[U];
            int64_t ip[U];
            TableDesc td[U];
#pragma unroll
            for (int uu = 0; uu < U; ++uu) {
                const int item = it0 + 256 * uu + tid;
                have[uu] = item < nitems;
                tt[uu] = have[uu] ? item / ppb1 : 0;
                const int col = (have[uu] ? item - tt[uu] * ppb1 : 0) * PL;
                c0[uu] = u0 + col;
                live[uu] = have[uu] && col < valid;
                td[uu] = load_table(tabs, tt[uu]);
                ip[uu] = tt[uu] * tstride + bA * L;
            }
            float sum[U][PL];
            for (int k0 = 0; k0 < Lr; k0 += KB) {
                int64_t ri[U][KB];
#pragma unroll
                for (int uu = 0; uu < U; ++uu)
#pragma unroll
                    for (int kk = 0; kk < KB; ++kk)
                        ri[uu][kk] = load_index_if(live[uu] && k0 + kk < L, idx, itype, ip[uu] + k0 + kk);
                const vt* src[U][KB];
#pragma unroll
                for (int uu = 0; uu < U; ++uu)
#pragma unroll
                    for (int kk = 0; kk < KB; ++kk) {
                        const bool use = live[uu] && k0 + kk < L;
                        const int64_t r = ri[uu][kk] - base;
                        const bool ok = use & (r >= 0) & (r < td[uu].nrows);
                        bad |= use & !ok & (c0[uu] == 0);
                        src[uu][kk] = ok ? (const vt*)((const T*)td[uu].data + r * d + c0[uu]) : zero;
                    }
                __builtin_amdgcn_sched_barrier(0);
                vt vv[U][KB];
#pragma unroll
                for (int uu = 0; uu < U; ++uu)
#pragma unroll
                    for (int kk = 0; kk < KB; ++kk) vv[uu][kk] = ldg<vt>(src[uu][kk]);
                __builtin_amdgcn_sched_barrier(0);
                // ---- phase B of unit u, under the row loads just issued
                if (doB && last_pass && k0 + KB >= Lr) gram(rt, nstepsB);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int uu = 0; uu < U; ++uu)
#pragma unroll
                    for (int kk = 0; kk < KB; ++kk) {
                        if (k0 + kk >= L) break;
                        float f[PL];
                        V::to_f32(vv[uu][kk], f);
#pragma unroll
                        for (int e = 0; e < PL; ++e) sum[uu][e] = (k0 + kk == 0) ? f[e] : sum[uu][e] + f[e];
                    }
            }
#pragma unroll
            for (int uu = 0; uu < U; ++uu) {
                if (!have[uu]) continue;
                const vt pooled = V::from_f32(sum[uu]);
                *(frag*)(wt + (tt[uu] + 1) * LD + (c0[uu] - u0)) = __builtin_bit_cast(frag, pooled);
                if (YS && live[uu]) stg<vt>(yrow + d + (int64_t)tt[uu] * d + c0[uu], pooled);
            }
            if (last_pass) break;
        }
        if (xc < vpad) {
            *(frag*)(wt + xc) = xf;
            if (xc < valid) {
                float f[PL];
                FR::to_f(f, xf);
#pragma unroll
                for (int k = 0; k < PL; ++k) stg<T>(orow + u0 + xc + k, from_f32<T>(f[k]));
                if (YS) stg<frag>(yrow + u0 + xc, xf);
            }
        }
        // ---- unit u was its sample's last block: Z[i][j], i > j, triangular_slice_kernel! order (i-major), after x
        if (doB && kB == nblk - 1) {
            T* zrow = out + bB * out_ld;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if (w + 4 * m >= NT) break;
                const f32x4_t z = NPART == 2 ? acc[0][m] + acc[NPART - 1][m] : acc[0][m];
                const int j = tJ[m] * 16 + c;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = tI[m] * 16 + 4 * q + r;
                    if (i < F && j < i) stg<T>(zrow + d + i * (i - 1) / 2 + j, from_f32<T>(z[r]));
                }
#pragma unroll
                for (int pp = 0; pp < NPART; ++pp) acc[pp][m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
            for (int e = d + P + tid; e < W; e += 256) stg<T>(zrow + e, from_f32<T>(0.0f));
        }
        if (doA && ++kA == nblk) {
            kA = 0;
            bA += gridDim.x;
        }
        if (doB && ++kB == nblk) {
            kB = 0;
            bB += gridDim.x;
        }
        __syncthreads();  // tile (u + 1) & 1 is complete, tile u & 1 is free
    }
    if (bad) raise_index_error(err);
}

template <typename T, bool YS>
static void launch_bags(hipStream_t s, unsigned grid, unsigned lds, int NB, const TableDesc* tabs, int d, int F, int B,
                        int CB, const void* x, int64_t x_ld, void* ys, int64_t ys_ld, void* out, int64_t out_ld,
                        int padding, const void* idx, int itype, int64_t tstride, int base, int L, unsigned* err) {
#define DLRM_BAGS_GO(NB_)                                                                                             \
    hipLaunchKernelGGL((bags_fwd_kernel<T, NB_, YS>), dim3(grid), dim3(256), lds, s, tabs, d, F, B, CB, (const T*)x, x_ld, \
                       (T*)ys, ys_ld, (T*)out, out_ld, padding, idx, itype, tstride, base, L, err)
    switch (NB) {
    case 1: DLRM_BAGS_GO(1); break;
    case 2: DLRM_BAGS_GO(2); break;
    case 3: DLRM_BAGS_GO(3); break;
    case 4: DLRM_BAGS_GO(4); break;
    case 5: DLRM_BAGS_GO(5); break;
    default: DLRM_BAGS_GO(6); break;
    }
#undef DLRM_BAGS_GO
}

int launch_bags_interact_fwd(dlrm_ctx* ctx, const TableDesc* tabs, bool tabs_aligned16, int T_, int dtype, const void* idx,
                             int itype, int64_t tstride, int base, int L, int d, int B, const void* x, int64_t x_ld,
                             void* ys, int64_t ys_ld, void* out, int64_t out_ld, int padding) {
    if (!bags_fused(dtype, d, T_, L, tabs_aligned16, x, x_ld, ys, ys_ld)) return DLRM_E_UNSUPPORTED;
    if (B == 0) return DLRM_OK;
    const int F = T_ + 1, NB = bags_nb(T_), CB = bags_cb_bytes(dtype, d, T_) / bags_esz(dtype);
    const unsigned lds = (unsigned)bags_lds_bytes(dtype, d, T_);
    // a workgroup per sample, as many per CU as are resident at once (registers, then the 160 KB of LDS); the rest
    // grid-strides, which is what gives a workgroup several units to pipeline
    const int by_lds = (int)(160 * 1024 / lds);
    const int per_cu = by_lds < bags_wg_per_cu(NB) ? (by_lds < 1 ? 1 : by_lds) : bags_wg_per_cu(NB);
    int64_t g = (int64_t)ctx_num_cus(ctx) * per_cu;
    if (g > B) g = B;
    const unsigned grid = (unsigned)(g < 1 ? 1 : g);
    hipStream_t s = ctx_stream(ctx);
    unsigned* err = ctx_error_word(ctx);
#define DLRM_BAGS_T(T, YS_)                                                                                            \
    launch_bags<T, YS_>(s, grid, lds, NB, tabs, d, F, B, CB, x, x_ld, ys, ys_ld, out, out_ld, padding, idx, itype, tstride, \
                        base, L, err)
    if (dtype == DLRM_F32) { if (ys) DLRM_BAGS_T(float, true); else DLRM_BAGS_T(float, false); }
    else { if (ys) DLRM_BAGS_T(uint16_t, true); else DLRM_BAGS_T(uint16_t, false); }
#undef DLRM_BAGS_T
    return ctx_hip(ctx, hipGetLastError(), "bags_interact_fwd launch");
}

}  // namespace dlrm
