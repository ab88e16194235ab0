// interact.hip — pairwise-dot feature interaction (DotInteraction) on gfx950 MFMA.
//
// Forward  = fast_vcat (src/model/interact.jl:271-281) + process_batches/process_slice!
//            (:449-467, :338-362): per sample Z = T T^T over the feature dim, then the strict
//            lower triangle in triangular_slice_kernel! order (:64-75), after x.
// Backward = process_batches_back (:469-489): S = symmetric zero-diagonal unpack of the
//            incoming gradient (:154-173), dT = S T (gemmavx!, :486), dx = dout_x + dT[0]
//            (sumavx, :434).  dT keeps the x rows, as dt_reshaped does (:428-435).
//
// One wave owns one sample.  T_b is [F][d] (F features padded to 16*NB rows), and the
// 16x16 MFMA tiles that hold the lower triangle of Z are the only ones computed:
//   fp32: v_mfma_f32_16x16x4_f32 — exact fp32 products with an fp32 fmaf chain.  Lane
//         (c = l&15, q = l>>4) loads one float4 of row 16I+c at columns u+4q..u+4q+3, and
//         component `comp` is its operand for k-step comp; since A and B of a Gram tile are
//         the same rows, one load feeds both operands of every tile pair (I, J<=I).
//   bf16: v_mfma_f32_16x16x32_bf16 — lane (c, q) holds 8 consecutive bf16 of row 16I+c at
//         columns 32u+8q.., again the same register for A and B; fp32 accumulate, one
//         rounding to bf16 on store (DotInteraction's scratchpads are Float32).
// The packed output row [x | pairs | 0-padding] is staged in LDS per wave and written
// back as one contiguous, coalesced run.
// Backward: dT (16NB x d) = S (16NB x 16NB) * T, with S built in LDS from the packed
// gradient (row stride = 16 mod 32 banks: conflict-free ds_read_b32 for the A fragments);
// B fragments are rows of T read straight from HBM (16 consecutive floats per 16 lanes).
// The interaction's arithmetic intensity (~11-24 flop/B) is far below the MFMA ridge, so
// these kernels are HBM-bound; MFMA just keeps the VALU free and the operand traffic low.
#include <cstdlib>
#include <string>
#include <type_traits>

#include "common.hpp"
#include "interact_plan.hpp"

#ifdef DLRM_PHASE
// Phase timestamps of the split indexer inside the step forward's launch (table DLRM_PHASE);
// only in the profiling variant of the library (tools/phase_stepfwd.py).
__device__ unsigned long long g_phase_fwd[64];
#define PHASE(k) do { __syncthreads(); if (blockIdx.x == DLRM_PHASE && threadIdx.x == 0) g_phase_fwd[k] = wall_clock64(); } while (0)
extern "C" int dlrm_debug_phase_fwd(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_fwd), sizeof(g_phase_fwd));
}
extern "C" int dlrm_debug_phase_fwd_reset(void) {
    static unsigned long long z[64];
    for (int k = 0; k < 64; ++k) z[k] = (k == 60 || k == 62) ? ~0ull : 0ull;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_phase_fwd), z, sizeof(z));
}
#endif
#include "indexer.hpp"

#ifdef DLRM_WTRACE
// Per-sample wave timestamps (wall_clock64, 100 MHz) of the forward (kind 0) and backward
// (kind 1) bodies; only in the tracing build (tools/wave_trace.sh).  Forward slots: 0 start,
// 1 indices returned, 2 first column step landed, 3 last column step landed, 4 MFMAs done,
// 5 output stores issued (the one-hot body stamps all six, fwd_onehot.hpp; the pooled body 0, 4, 5).  Backward
// slots: the kernels' text 0..4 (start, S barrier, MFMAs done, stores issued, stores drained), bwd_split_tracked
// its seven (BWTS_FLUSH).
__device__ unsigned long long g_wt[2][7][8192];
#define WT(kind, slot, b) do { if ((threadIdx.x & 63) == 0 && (b) < 8192) g_wt[kind][slot][b] = wall_clock64(); } while (0)
extern "C" int dlrm_debug_wtrace(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wt), sizeof(g_wt));
}
extern "C" int dlrm_debug_wtrace_slots(void) { return 7; }
#else
#define WT(kind, slot, b) do {} while (0)
#endif

#include "fwd_onehot.hpp"
#include "apply.hpp"  // the split rule's step (split_step, Halves)

namespace dlrm {

// Workgroup `bid` of `nblocks` (WPB waves, one sample per wave); stage_all = WPB * kStage floats of LDS.
// The fused one-hot forward of F <= 32 features reads its table pointers from a TabPtrs kernel
// argument (fwd_onehot.hpp); kDeferRaise: its bounds flag is raised after the stores.
#ifndef DLRM_DEFER_RAISE
#define DLRM_DEFER_RAISE 1
#endif
constexpr bool kDeferRaise = DLRM_DEFER_RAISE;
// Column steps of row loads a wave of the one-hot forward keeps in flight (fwd_onehot.hpp, WIN;
// 0: all of a column block).  The rolling window is chosen per instantiation, where it was measured
// to win in the training step: three of the eight steps for the fused fp32 lookup + interaction of
// 17..32 features at d = 128 (DLRM_FWD_WIN builds another window there; DESIGN.md section 3: 2, 3, 4
// and 6 measured).  Every other instantiation keeps every step in flight.
#ifndef DLRM_FWD_WIN
#define DLRM_FWD_WIN 3
#endif
template <typename T, int NB, bool FUSED, int DC> constexpr int fwd_window() {
    return (std::is_same<T, float>::value && NB == 2 && FUSED && DC == 128) ? DLRM_FWD_WIN : 0;
}
template <int NB, bool FUSED, bool POOL> constexpr bool fwd_tab_ptrs() { return FUSED && !POOL && NB <= 2; }

template <typename T, int NB, bool FUSED, int WPB, bool POOL = false, int DC = 0, int WIN = 0>
__device__ __forceinline__ void fwd_body(int bid, int nblocks, float* stage_all, int d_, int F, int B,
                                         const T* __restrict__ x, int64_t x_ld, T* __restrict__ ys, int64_t ys_ld,
                                         T* __restrict__ out, int64_t out_ld, int padding, const GatherArgs& ga,
                                         const TabPtrs* tp = nullptr) {
    // !POOL: one lookup per (table, sample) -- the callers pick the POOL kernel for FUSED, L > 1
    if constexpr (!POOL) {
        // one wave per sample: with the table pointers in the kernel arguments it beats two waves per
        // sample (column halves) at d = 128 -- tools/fwd_probe.hip: 10.5 vs 11.9 us
        constexpr int WPS = 1;
        constexpr bool TP = fwd_tab_ptrs<NB, FUSED, POOL>();
        fwd_body_onehot<T, NB, FUSED, WPB, DC, WPS, false, TP, kDeferRaise && TP, WIN>(
            bid, nblocks, stage_all, d_, F, B, x, x_ld, ys, ys_ld, out, out_ld, padding, ga, tp);
        return;
    }
    const int d = DC > 0 ? DC : d_;  // DC: the feature size as a compile-time constant
    typedef Frag<T> FR;
    typedef typename FR::type frag;
    constexpr int UU = 128 / FR::COLS;  // column steps whose loads are issued together (128 columns)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int P = F * (F - 1) / 2;
    const int W = d + P + padding;
    const bool staged = W <= kStage;
    float* stage = stage_all + w * kStage;
    for (int64_t b = (int64_t)bid * WPB + w; b < B; b += (int64_t)nblocks * WPB) {
        WT(0, 0, b);
        const T* xb = x + b * x_ld;
        T* yb = ys ? ys + b * ys_ld : nullptr;  // FUSED: ys may be NULL (not materialized)
        T* orow = out + b * out_ld;
        // fast_vcat: x into the reserved rows of ys; x is also the head of the output row.
        for (int i = lane; i < d; i += 64) {
            const T v = ldg<T>(xb + i);
            if (yb) stg<T>(yb + i, v);
            if (staged) stage[i] = to_f32(v);
            else stg<T>(orow + i, v);
        }
        // row sources: feature 0 is x itself; features 1..F-1 are ys rows or table rows.  Every
        // load below executes unconditionally (invalid slots read x and are masked to zero), so
        // no branch makes the compiler wait for a lane's loads one at a time.
        const T* src[NB];
        int64_t kidx[NB];  // FUSED, pooled: index position of lookup 0 of this (table, sample)
        TableDesc td[NB];
#pragma unroll
        for (int I = 0; I < NB; ++I) {
            const int row = I * 16 + c;
            const bool tab = FUSED && row >= 1 && row < F;
            kidx[I] = tab ? (row - 1) * ga.tstride + b * ga.L : -1;
            td[I] = FUSED ? load_table(ga.tabs, tab ? row - 1 : 0) : TableDesc{};
            const int64_t r = load_index_if(tab, ga.idx, ga.itype, kidx[I]) - ga.base;
            const bool ok = tab & (r >= 0) & (r < td[I].nrows);
            if (tab & !ok & (q == 0)) raise_index_error(ga.err);
            src[I] = row == 0 ? xb
                              : (!FUSED ? (row < F ? yb + (int64_t)row * d : nullptr)
                                        : (ok ? (const T*)td[I].data + r * d : nullptr));
        }
        f32x4_t acc2[NB <= 2 ? 2 : 1][NB * (NB + 1) / 2];  // NB <= 2: parity partials (fwd_body_onehot's order)
#pragma unroll
        for (int k = 0; k < NB * (NB + 1) / 2; ++k) acc2[0][k] = acc2[NB <= 2 ? 1 : 0][k] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        for (int u0 = 0; u0 < d; u0 += UU * FR::COLS) {
            frag a[UU][NB];
#pragma unroll
            for (int uu = 0; uu < UU; ++uu) {
                const int col = u0 + uu * FR::COLS + q * FR::PER_LANE;
#pragma unroll
                for (int I = 0; I < NB; ++I) {
                    const bool ok = src[I] && col < d;
                    // F <= 32, one-hot: column steps past d (small d, wave-uniform) issue no load at all
                    // (D = 16: 9.5 vs 11.0 us).  Not in the pooled or NB > 2 kernels, where the branches
                    // halve the loads kept in flight (the NB = 5 forward: 105 vs 72 us at d = 256).
                    const frag v = (POOL || NB > 2 || u0 + uu * FR::COLS < d)
                                       ? ldg<frag>((ok ? src[I] : xb) + (ok ? col : 0))
                                       : FR::zero();
                    a[uu][I] = ok ? v : FR::zero();
                }
            }
            if (FUSED) {
                // pooled bags: add lookups 1..L-1 in k order (fp32), round once to T
                if (POOL && ga.L > 1) {
#pragma unroll
                    for (int I = 0; I < NB; ++I) {
                        const bool tab = kidx[I] >= 0;
                        float f[UU][FR::PER_LANE];
#pragma unroll
                        for (int uu = 0; uu < UU; ++uu) FR::to_f(f[uu], a[uu][I]);
#pragma unroll 4
                        for (int k = 1; k < ga.L; ++k) {
                            const int64_t r = load_index_if(tab, ga.idx, ga.itype, kidx[I] + k) - ga.base;
                            const bool ok = tab & (r >= 0) & (r < td[I].nrows);
                            if (tab & !ok & (q == 0) & (u0 == 0)) raise_index_error(ga.err);
                            const T* rp = ok ? (const T*)td[I].data + r * d : xb;
#pragma unroll
                            for (int uu = 0; uu < UU; ++uu) {
                                const int col = u0 + uu * FR::COLS + q * FR::PER_LANE;
                                const bool okc = ok && col < d;
                                const frag v = ldg<frag>(rp + (okc ? col : 0));
                                FR::add_to(f[uu], okc ? v : FR::zero());
                            }
                        }
#pragma unroll
                        for (int uu = 0; uu < UU; ++uu) a[uu][I] = FR::from_f(f[uu]);
                    }
                }
                // the lookup output: ys rows 1..F-1 written from the fragments
                if (yb)
#pragma unroll
                for (int uu = 0; uu < UU; ++uu) {
                    const int col = u0 + uu * FR::COLS + q * FR::PER_LANE;
#pragma unroll
                    for (int I = 0; I < NB; ++I) {
                        const int row = I * 16 + c;
                        if (row >= 1 && row < F && col < d) stg<frag>(yb + (int64_t)row * d + col, a[uu][I]);
                    }
                }
            }
#pragma unroll
            for (int uu = 0; uu < UU; ++uu) {
                int ij = 0;
#pragma unroll
                for (int I = 0; I < NB; ++I)
#pragma unroll
                    for (int J = 0; J <= I; ++J, ++ij) FR::mma(acc2[NB <= 2 ? (uu & 1) : 0][ij], a[uu][I], a[uu][J]);
            }
        }
        f32x4_t acc[NB * (NB + 1) / 2];
#pragma unroll
        for (int k = 0; k < NB * (NB + 1) / 2; ++k) acc[k] = NB <= 2 ? acc2[0][k] + acc2[1][k] : acc2[0][k];
        WT(0, 4, b);
        // Z[i][j], i > j: triangular_slice_kernel! order (i-major), after x
        {
            int ij = 0;
#pragma unroll
            for (int I = 0; I < NB; ++I)
#pragma unroll
                for (int J = 0; J <= I; ++J, ++ij) {
                    const int j = J * 16 + c;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = I * 16 + 4 * q + r;
                        if (i < F && j < i) {
                            const int e = d + i * (i - 1) / 2 + j;
                            if (staged) stage[e] = acc[ij][r];
                            else stg<T>(orow + e, from_f32<T>(acc[ij][r]));
                        }
                    }
                }
        }
        for (int e = d + P + lane; e < W; e += 64) {
            if (staged) stage[e] = 0.0f;
            else stg<T>(orow + e, from_f32<T>(0.0f));
        }
        if (staged) {
            wave_lds_sync();
            for (int e = lane; e < W; e += 64) stg<T>(orow + e, from_f32<T>(stage[e]));
            wave_lds_sync();
        }
        WT(0, 5, b);
    }
}

// POOL: the pooled-bag path (lookups > 1) is compiled in; the one-hot kernel stays lean.
template <typename T, int NB, bool FUSED, bool POOL, int DC = 0, int WPB = 4>
__global__ __launch_bounds__(64 * WPB, 2) void interact_fwd_kernel(int d, int F, int B, const T* __restrict__ x,
                                                                   int64_t x_ld, T* __restrict__ ys, int64_t ys_ld,
                                                                   T* __restrict__ out, int64_t out_ld, int padding,
                                                                   GatherArgs ga, TabPtrs tp) {
    __shared__ __attribute__((aligned(16))) float stage_all[WPB * kStage];
    fwd_body<T, NB, FUSED, WPB, POOL, DC, fwd_window<T, NB, FUSED, DC>()>(blockIdx.x, gridDim.x, stage_all, d, F, B, x, x_ld,
                                                                          ys, ys_ld, out, out_ld, padding, ga, &tp);
}

// The forward of a training step with the SparseIndexer build in the same grid (split form:
// once-hit positions flagged for the backward, the rest listed for the apply): the first
// T << ix.vshift workgroups sort the tables' positions (indexer.hpp, 256 threads; with
// vshift = 1 two per table, one per row parity, which halves the critical path), the rest run
// the fused lookup + interaction without ys.  The indexer depends only on the indices, so it
// streams beside the gather instead of adding a launch.
// (StepLds, kStepIndexEPL: indexer.hpp)
template <typename T, int NB, int DC = 0>
__global__ __launch_bounds__(256, 3) void interact_fwd_index_kernel(int d, int F, int B, const T* __restrict__ x,
                                                                 int64_t x_ld, T* __restrict__ out, int64_t out_ld,
                                                                 int padding, GatherArgs ga, IndexerDev ix,
                                                                 TabPtrs tp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int T_ = F - 1;
    // vshift >= 2: the wave build (indexer.hpp wave_build_group: 4 parts per workgroup, one wave
    // each, and the flat item map); else the block build, one workgroup per table part
    const bool wave = ix.vshift >= 2;
    const int NI = wave ? (T_ << ix.vshift) / kWaveParts : T_ << ix.vshift;
#ifdef DLRM_PHASE
    // [0] this block's start (the traced indexer block), [60] / [61] first start / last end of any
    // gather block, [62] / [63] first start / last end of any indexer block
    if (threadIdx.x == 0) {
        const unsigned long long t0 = wall_clock64();
        if ((int)blockIdx.x == DLRM_PHASE) g_phase_fwd[0] = t0;
        atomicMin(&g_phase_fwd[(int)blockIdx.x < NI ? 62 : 60], t0);
    }
#endif
    if ((int)blockIdx.x < NI) {
        if (wave) {
            wave_build_group<false>(ix, blockIdx.x, T_, ga.tabs, ga.idx, ga.itype, ga.tstride, ga.base, B * ga.L, ga.err,
                             *(WaveBuildLds*)smem);
        } else {
            StepLds& sl = *(StepLds*)smem;
            const int v = blockIdx.x, t = v >> ix.vshift;
            fast_index_table<256, kStepIndexEPL, true>(ix, v, t, ix.vshift, (uint32_t)ga.tabs[t].nrows, ga.idx,
                                                       ga.itype, ga.tstride, ga.base, B * ga.L, ga.err, sl);
        }
#ifdef DLRM_PHASE
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(&g_phase_fwd[63], wall_clock64());
#endif
        return;
    }
    fwd_body<T, NB, true, 4, false, DC>(blockIdx.x - NI, gridDim.x - NI, smem, d, F, B, x, x_ld, nullptr, 0, out,
                                        out_ld, padding, ga, &tp);
#ifdef DLRM_PHASE
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&g_phase_fwd[61], wall_clock64());
#endif
}

// ---------------------------------------------------------------------------------- bwd
template <int NB> struct BwdGeom {
    static constexpr int NS = 16 * NB;                          // padded features
    static constexpr int SS = NS + ((NB % 2 == 0) ? 16 : 0);    // row stride = 16 (mod 32)
    static constexpr int WPB = NB <= 2 ? 4 : (NB <= 4 ? 2 : 1); // waves per block
    static constexpr int LDS_FLOATS = NS * SS;                  // per wave: S
    // per wave, with the UPD T tile ([NS][64] floats of one super-block) after S
    template <bool UPD> static constexpr int lds_floats() { return NS * SS + (UPD ? NS * 64 : 0); }
};

// 4 consecutive elements of T as fp32 (16-B load for fp32, 8-B for bf16)
__device__ __forceinline__ f32x4_t load4_f32(const float* p) { return ldg<f32x4_t>(p); }
__device__ __forceinline__ f32x4_t load4_f32(const uint16_t* p) {
    const uint2 v = ldg<uint2>(p);
    return f32x4_t{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16),
                   __uint_as_float(v.y & 0xffff0000u)};
}

// dT = S T per sample, in 64-column super-blocks: lane (c, q) loads T[4s+q][64sb+4c .. +3]
// (16 lanes read 256 contiguous bytes of a row), and component e of that float4 is the B
// operand of the MFMA that produces output columns 64sb + 4j + e.  The four accumulators of
// a tile row then hold 4 consecutive output columns per lane -> one float4 store per row.
// All k-step loads of a super-block are issued before its MFMAs (up to 4*NB in flight).
// GATHER: T_b is not read from a materialized ys but rebuilt from x (row 0) and the table
// rows of the sample's one-hot indices (rows 1..F-1): the same values, without ys.
// UPD (training step, split indexer): a table row hit by this sample only (single[] flag of
// the forward's indexer build) gets its SGD step here -- w = fmaf(-lr, 0 + g, w), exactly the
// apply kernel's arithmetic for a one-position segment -- and its dt row is not written.  No
// other sample reads that row, so the in-place update cannot race with another wave's gather.
struct StepUpdate {
    const uint8_t* single;  // [T][cap]
    int64_t cap;
    float lr;
    const unsigned* err;    // the ctx's bounds flag: set -> no table row is written (the row goes to dt)
    // What differs between the rules is theirs: the kind (kSplit; kAdagrad 1: element-wise, 2: row-wise), and for a
    // rule whose rows have a second stream (low halves, Adagrad state) that stream's element type State and the
    // tables' pointers to it, a member `state`; kName heads the launch errors.
    static constexpr bool kSplit = false;
    static constexpr int kAdagrad = 0;
    static constexpr bool kStochastic = false;
    typedef void State;
    static constexpr const char* kName = "step_bwd";
};
// The same for split-bf16 tables (apply.hpp SplitDescent; dlrm_split_step_bwd): the table holds the high
// halves of fp32 master weights, lo[t] their low halves.  A once-hit row's master weight is merged from
// the gathered bf16 element (the wave's tile holds it exactly, as bf16 bits or as their fp32 value) and
// its low half, stepped in fp32 and written back as two halves.  A struct of its own, so the Descent
// kernels keep their arguments.
struct SplitStepUpdate : StepUpdate {
    uint16_t* const* state;  // [T] device pointers to the low halves, uint16 [nrows][d]
    static constexpr bool kSplit = true;
    typedef uint16_t State;
    static constexpr const char* kName = "split_step_bwd";
};

// The same for the sparse Adagrad rules (apply.hpp Adagrad / RowwiseAdagrad; dlrm_adagrad_step_bwd): a once-hit
// row's fp32 state (RW: one word per row, else a row of d) is loaded after the MFMAs, stepped with the apply's
// own helpers on G = 0 + g, and written with the row.  A struct of its own again.
template <bool RW>
struct AdagradStepUpdate : StepUpdate {
    float* const* state;    // [T] device pointers, fp32 [nrows][d] or (RW) [nrows]
    float eps;
    static constexpr int kAdagrad = RW ? 2 : 1;
    typedef float State;
    static constexpr const char* kName = "adagrad_step_bwd";
};

// The same for the stochastic rule on bf16 tables (apply.hpp StochasticDescent; dlrm_sr_step_bwd): Descent's write
// with the rule's store -- w = sr_bf16(fmaf(-lr, 0 + g, w), R), R the 16 Philox bits of (seed, step, table, row,
// column) that the apply's once-hit item draws for the element, generated at the write, after the MFMAs.  No second
// stream: the seed's halves and the pointer to the handle's step word, which each workgroup reads once
// (StochasticDescent::load_step).  A struct of its own again.
struct StochasticStepUpdate : StepUpdate {
    uint32_t k0, k1;       // the seed's halves
    const uint64_t* step;  // the handle's step word
    static constexpr bool kStochastic = true;
    static constexpr const char* kName = "sr_step_bwd";
};

// The same for the sparse Adagrad rules with the stochastic store on bf16 tables (apply.hpp StochasticAdagrad /
// StochasticRowwiseAdagrad; dlrm_sr_adagrad_step_bwd): AdagradStepUpdate's arithmetic and state write, the weights
// stored by SrWord::store -- sr_bf16(W', R), R as the apply's once-hit item draws it, generated at the write.  The
// parent's fields, then the seed's halves and the pointer to the handle's step word (read once per workgroup).  A
// struct of its own again.
template <bool RW>
struct StochasticAdagradStepUpdate : AdagradStepUpdate<RW> {
    uint32_t k0, k1;       // the seed's halves
    const uint64_t* step;  // the handle's step word
    static constexpr bool kStochastic = true;
    static constexpr const char* kName = "sr_adagrad_step_bwd";
};

// the d = 128 rule kernels' per-table pointers to the second stream in LDS, and the row-wise two-wave form's
// exchange of each wave's sums of squares (function-local arrays: only their instantiations hold them)
template <typename E, int N> __device__ __forceinline__ E** rule_tab() {
    __shared__ E* t[N];
    return t;
}
// interact_bwd_split_kernel reads a rule's pointer array through this call by reference, not as su.state in its own
// text: read there, every rule kernel kept its instruction count and resource figures, but one scalar `and` of each
// had its operands the other way round and the 8-column forms ordered a few instructions differently
// (DESIGN.md section 16).
template <typename SU> __device__ __forceinline__ typename SU::State* const* rule_state(const SU& su) { return su.state; }
template <int N> __device__ __forceinline__ float* row_ss_tab() {
    __shared__ float t[N];
    return t;
}

// N once-hit elements of a split row: hb = the gathered high halves as fp32 bits (bf16 << 16), lv the low
// halves, g the gradient; w = fmaf(-lr, 0 + g, w) on the merged weight (split_step1: the apply's singles
// arithmetic, NaN quiet-bit rule included), both halves stored.
template <int N>
__device__ __forceinline__ void split_once_hit(float lr, const float* g, const uint32_t* hb, typename Halves<N>::type lv,
                                               uint16_t* hrow, uint16_t* lrow) {
    typename Halves<N>::type hv;
    float gg[N];
#pragma unroll
    for (int e = 0; e < N; ++e) {
        hv[e] = (uint16_t)(hb[e] >> 16);
        gg[e] = 0.0f + g[e];
    }
    split_step<N>(lr, gg, hv, lv);
    stg_nt<typename Halves<N>::type>(hrow, hv);
    stg_nt<typename Halves<N>::type>(lrow, lv);
}

template <typename T, int NB, bool GATHER, bool UPD = false, int SBU_ = 0, int DC = 0, typename SU = StepUpdate>
__device__ __forceinline__ void bwd_body(int bid, int nblocks, float* smem, int d_, int F, int B,
                                         const T* __restrict__ dout, int64_t dout_ld, const T* __restrict__ t,
                                         int64_t t_ld, float* __restrict__ dx, int64_t dx_ld,
                                         float* __restrict__ dt, int64_t dt_ld, const GatherArgs& ga,
                                         const T* __restrict__ x, int64_t x_ld, const SU& su = SU{}) {
    const int d = DC > 0 ? DC : d_;  // DC: the feature size as a compile-time constant
    typedef BwdGeom<NB> G;
    constexpr int KS = 4 * NB;          // max k-steps (F <= 16 NB)
    constexpr int SBU = SBU_ > 0 ? SBU_ : (NB <= 2 ? 2 : 1);  // 64-column super-blocks loaded together
    constexpr int KPB = 8;              // packed-gradient values per lane loaded together
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // the table descriptors, once per workgroup, in LDS after the waves' regions: read where
    // used instead of held in registers across the index loads
    TableDesc* tds = (TableDesc*)(smem + G::WPB * G::template lds_floats<UPD>());
    int64_t* dmap = (int64_t*)(tds + (F - 1));  // GATHER + ga.dtb: [2][F-1] row bases / strides of dt
    typedef typename SU::State SE;
    SE** sop = (SE**)(tds + (F - 1));  // the split step (no dtb): [F-1] low-half pointers
    if (GATHER) {
        for (int t = threadIdx.x; t < F - 1; t += blockDim.x) {
            tds[t] = load_table(ga.tabs, t);
            if constexpr (SU::kSplit) sop[t] = ldg<SE*>(su.state + t);
            if (ga.dtb) {
                dmap[t] = ga.dtb[t];
                dmap[F - 1 + t] = ga.dtl[t];
            }
        }
        __syncthreads();
    }
    const bool mapped = GATHER && ga.dtb;
    if (w >= G::WPB) return;
    const int c = lane & 15, q = lane >> 4;
    float* S = smem + w * G::template lds_floats<UPD>();
    float* Tt = S + G::NS * G::SS;  // UPD: the current super-block of T, [NS][64]
    const int P = F * (F - 1) / 2;
    const int ksteps = (F + 3) / 4;
    for (int64_t b = (int64_t)bid * G::WPB + w; b < B; b += (int64_t)nblocks * G::WPB) {
        WT(1, 0, b);
        const T* ob = dout + b * dout_ld;
        const T* tb = GATHER ? nullptr : t + b * t_ld;
        // Independent loads first, so their latencies overlap: the sample's indices (T rows and,
        // UPD, the once-hit flags of its output rows) and the first packed-gradient values.
        const T* rowp[KS];  // GATHER: this lane's T rows kk = 4s + q
        if (GATHER) {
            int64_t ri[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int kk = 4 * s + q;
                const bool tab = s < ksteps && kk >= 1 && kk < F;
                ri[s] = load_index_if(tab, ga.idx, ga.itype, (kk - 1) * ga.tstride + b * ga.L);
            }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const int kk = 4 * s + q;
                const bool tab = s < ksteps && kk >= 1 && kk < F;
                const TableDesc td = tds[tab ? kk - 1 : 0];
                const int64_t r = ri[s] - ga.base;
                const bool ok = tab & (r >= 0) & (r < td.nrows);
                if (tab & !ok & (c == 0)) raise_index_error(ga.err);
                rowp[s] = (s < ksteps && kk == 0) ? x + b * x_ld : (ok ? (const T*)td.data + r * d : nullptr);
            }
        }
        uint32_t urow[NB][4];  // UPD: the once-hit table row of output row f = 16I + 4q + r, else ~0u
        if (UPD) {
            // a bounds error of this step (raised by the forward): the reference's gather throws
            // before update!, so every row goes to dt and the apply (which checks too) writes none
            const bool frozen = *su.err != 0;
            if (b == 0 && lane == 0) snapshot_error(su.err, frozen ? 1u : 0u);
            uint8_t fl[NB][4];
            int64_t ui[NB][4];
#pragma unroll
            for (int I = 0; I < NB; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = I * 16 + 4 * q + r;
                    const bool tab = f >= 1 && f < F;
                    fl[I][r] = ldg<uint8_t>(su.single + (tab ? (int64_t)(f - 1) * su.cap + b : 0));
                    ui[I][r] = load_index_if(tab, ga.idx, ga.itype, (f - 1) * ga.tstride + b);
                }
#pragma unroll
            for (int I = 0; I < NB; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = I * 16 + 4 * q + r;
                    const bool tab = f >= 1 && f < F;
                    const TableDesc td = tds[tab ? f - 1 : 0];
                    const int64_t rr = ui[I][r] - ga.base;
                    urow[I][r] = (tab & !frozen & (fl[I][r] != 0) & (rr >= 0) & (rr < td.nrows)) ? (uint32_t)rr : ~0u;
                }
        }
        // The first super-blocks' T rows (and dout's x part) go out before S is built, so their
        // latency overlaps the packed-gradient loads and the LDS scatter.
        f32x4_t bv[SBU][KS];
        f32x4_t xo[SBU];
        // every lane's T row pointer is valid (ob, the dout row, stands in for a missing row) and
        // `live` masks the values, so the loads are plain base + offset with no selects
        unsigned live = 0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int kk = 4 * s + q;
            const T* src = GATHER ? rowp[s] : (kk < F ? tb + (int64_t)kk * d : nullptr);
            live |= (s < ksteps && src) ? (1u << s) : 0u;
            rowp[s] = (s < ksteps && src) ? src : ob;
        }
        auto load_batch = [&](int sb0) {
#pragma unroll
            for (int h = 0; h < SBU; ++h) {
                const int n0 = sb0 + 64 * h + 4 * c;
                const int nc = n0 < d ? n0 : 0;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const f32x4_t v = load4_f32(rowp[s] + nc);
                    bv[h][s] = ((live >> s) & 1u) && n0 < d ? v : f32x4_t{0.f, 0.f, 0.f, 0.f};
                }
                const int nx = n0 < d ? n0 : 0;  // dout rows need no alignment: scalar reads
                xo[h] = f32x4_t{to_f32(ldg<T>(ob + nx)), to_f32(ldg<T>(ob + nx + 1)), to_f32(ldg<T>(ob + nx + 2)),
                                to_f32(ldg<T>(ob + nx + 3))};
            }
        };
        load_batch(0);
        // S: zero, then scatter the packed pairs to both triangles (fused unpack + transpose-add);
        // KPB values per lane in flight
        for (int e = lane; e < G::NS * G::NS; e += 64) S[(e / G::NS) * G::SS + (e % G::NS)] = 0.0f;
        wave_lds_sync();
        for (int p0 = 0; p0 < P; p0 += 64 * KPB) {
            float dv[KPB];
#pragma unroll
            for (int k = 0; k < KPB; ++k) {
                const int p = p0 + 64 * k + lane;
                const float v = to_f32(ldg<T>(ob + d + (p < P ? p : 0)));
                dv[k] = p < P ? v : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < KPB; ++k) {
                const int p = p0 + 64 * k + lane;
                if (p < P) {
                    int i = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
                    while (i * (i - 1) / 2 > p) --i;
                    while ((i + 1) * i / 2 <= p) ++i;
                    const int j = p - i * (i - 1) / 2;
                    S[i * G::SS + j] = dv[k];
                    S[j * G::SS + i] = dv[k];
                }
            }
        }
        wave_lds_sync();
        WT(1, 1, b);
        for (int sb0 = 0; sb0 < d; sb0 += 64 * SBU) {
            if (sb0 > 0) load_batch(sb0);
#pragma unroll
            for (int h = 0; h < SBU; ++h) {
                const int sb = sb0 + 64 * h;
                if (sb >= d) break;
                const int n0 = sb + 4 * c;  // this lane's 4 output columns
                const bool colok = n0 < d;
                if (UPD) {  // stage the super-block's T rows: the update needs row f where dt row f is
                    wave_lds_sync();
#pragma unroll
                    for (int s = 0; s < KS; ++s) {
                        const int kk = 4 * s + q;
                        if (s < ksteps && kk < F) *(f32x4_t*)(Tt + kk * 64 + 4 * c) = bv[h][s];
                    }
                    wave_lds_sync();
                }
                f32x4_t acc[NB][4];
#pragma unroll
                for (int I = 0; I < NB; ++I)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[I][e] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    if (s < ksteps) {
                        const int kk = 4 * s + q;
#pragma unroll
                        for (int I = 0; I < NB; ++I) {
                            const float av = S[kk * G::SS + I * 16 + c];  // = S[16I+c][kk] (symmetric)
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                acc[I][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[h][s][e], acc[I][e], 0, 0, 0);
                        }
                    }
                }
                if (sb < 128) WT(1, 2 + sb / 64, b);
                if (colok) {
#pragma unroll
                    for (int I = 0; I < NB; ++I)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int f = I * 16 + 4 * q + r;
                            if (f < F) {
                                const f32x4_t v = f32x4_t{acc[I][0][r], acc[I][1][r], acc[I][2][r], acc[I][3][r]};
                                if (UPD && urow[I][r] != ~0u) {
                                    const f32x4_t tw = *(const f32x4_t*)(Tt + f * 64 + 4 * c);
                                    if constexpr (SU::kSplit) {
                                        const int64_t ro = (int64_t)urow[I][r] * d + n0;
                                        const float g4[4] = {v[0], v[1], v[2], v[3]};
                                        const uint32_t hb[4] = {__float_as_uint(tw[0]), __float_as_uint(tw[1]),
                                                                __float_as_uint(tw[2]), __float_as_uint(tw[3])};
                                        split_once_hit<4>(su.lr, g4, hb, load_halves<4>(sop[f - 1] + ro),
                                                          (uint16_t*)tds[f - 1].data + ro, sop[f - 1] + ro);
                                    } else {
                                    float wv[4];
#pragma unroll
                                    for (int e = 0; e < 4; ++e) wv[e] = __builtin_fmaf(-su.lr, 0.0f + v[e], tw[e]);
                                    store_row<T, 4>((T*)tds[f - 1].data + (int64_t)urow[I][r] * d, n0, wv);
                                    }
                                } else if (!mapped) {
                                    stg<f32x4_t>(dt + b * dt_ld + (int64_t)f * d + n0, v);
                                } else if (f > 0) {
                                    stg<f32x4_t>(dt + dmap[f - 1] + b * dmap[F - 2 + f] + n0, v);
                                }
                                if (f == 0) stg<f32x4_t>(dx + b * dx_ld + n0, xo[h] + v);
                            }
                        }
                }
            }
        }
        WT(1, 4, b);
        wave_lds_sync();
    }
}

template <typename T, int NB, bool GATHER>
__global__ __launch_bounds__(256, 2) void interact_bwd_kernel(int d, int F, int B, const T* __restrict__ dout,
                                                           int64_t dout_ld, const T* __restrict__ t, int64_t t_ld,
                                                           float* __restrict__ dx, int64_t dx_ld,
                                                           float* __restrict__ dt, int64_t dt_ld, GatherArgs ga,
                                                           const T* __restrict__ x, int64_t x_ld) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    bwd_body<T, NB, GATHER>(blockIdx.x, gridDim.x, smem, d, F, B, dout, dout_ld, t, t_ld, dx, dx_ld, dt, dt_ld, ga,
                            x, x_ld);
}

// The backward of a training step with the SparseIndexer build in the same grid: workgroups
// [0, T) each sort one table's positions (indexer.hpp, 256 threads, while the backward's
// workgroups stream), the rest run the re-gathering backward.  Occupancy 3 per SIMD leaves
// room for the indexer's workgroups beside the backward's two per CU.
constexpr int kBwdIndexEPL = 8;  // positions per thread: N <= 2048
template <typename T, int NB>
__global__ __launch_bounds__(256, 3) void interact_bwd_index_kernel(int d, int F, int B, const T* __restrict__ dout,
                                                                    int64_t dout_ld, float* __restrict__ dx,
                                                                    int64_t dx_ld, float* __restrict__ dt,
                                                                    int64_t dt_ld, GatherArgs ga,
                                                                    const T* __restrict__ x, int64_t x_ld,
                                                                    IndexerDev ix) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int T_ = F - 1;
    if ((int)blockIdx.x < T_) {
        FastLds<256, kBwdIndexEPL>& sl = *(FastLds<256, kBwdIndexEPL>*)smem;
        fast_index_table<256, kBwdIndexEPL>(ix, blockIdx.x, blockIdx.x, 0, (uint32_t)ga.tabs[blockIdx.x].nrows,
                                            ga.idx, ga.itype, ga.tstride, ga.base, B * ga.L, ga.err, sl);
        return;
    }
    bwd_body<T, NB, true, false, 1>(blockIdx.x - T_, gridDim.x - T_, smem, d, F, B, dout, dout_ld, nullptr, 0, dx, dx_ld, dt,
                          dt_ld, ga, x, x_ld);
}

// The backward of a training step after interact_fwd_index_kernel: re-gathers T, writes dx
// and the dt rows of positions whose row is hit more than once, and applies the SGD step to
// once-hit rows itself (the apply launch that follows handles the rest).  SU: Descent's rule or the split rule's.
template <typename T, int NB, int SBU, int DC = 0, typename SU = StepUpdate>
__global__ __launch_bounds__(256, 2) void interact_bwd_update_kernel(int d, int F, int B, const T* __restrict__ dout,
                                                                  int64_t dout_ld, float* __restrict__ dx,
                                                                  int64_t dx_ld, float* __restrict__ dt, int64_t dt_ld,
                                                                  GatherArgs ga, const T* __restrict__ x, int64_t x_ld,
                                                                  SU su) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    bwd_body<T, NB, true, true, SBU, DC, SU>(blockIdx.x, gridDim.x, smem, d, F, B, dout, dout_ld, nullptr, 0, dx, dx_ld,
                                             dt, dt_ld, ga, x, x_ld, su);
}

// The instantiations of interact_bwd_split_kernel (below) that run bwd_split_tracked's schedule: Descent on fp32
// tables at d = 128, two waves per sample, the step's own dt layout (the metric step's backward, 1 or 2 row blocks).
// Every other instantiation keeps the kernel's text.
template <typename T, int DC, int WPS, bool MAPPED, int CPL, bool YS, typename SU> constexpr bool bwd_tracked() {
    return std::is_same<T, float>::value && DC == 128 && WPS == 2 && CPL == 4 && !MAPPED && !YS && !SU::kSplit &&
           SU::kAdagrad == 0 && !SU::kStochastic;
}

#ifdef DLRM_WTRACE
// Backward stamps: held in registers and written after the wave's last store, so no stamp's store sits in the
// in-order vmcnt queue of the row loads.  Slots: 0 start, 1 indices back, 2 first row load issued, 3 first step
// landed, 4 last step landed, 5 MFMAs done, 6 last store issued.
#define BWTS_FLUSH(b) do { if ((threadIdx.x & 63) == 0 && (b) < 8192) { _Pragma("unroll") for (int s_ = 0; s_ < 7; ++s_) g_wt[1][s_][b] = wts_[s_]; } } while (0)
#else
#define BWTS_FLUSH(b) do {} while (0)
#endif

// interact_bwd_split_kernel's work for the bwd_tracked forms (one 64-column super-block per wave, wave h of a
// sample the columns 64h ..), with the dependent chains between its phases cut:
//  - lane t loads table t's descriptor itself, beside its index and flag, validates its index and forms its row's
//    address in-lane; the row addresses (and later the once-hit rows' store addresses) reach their lanes by
//    shuffles of that address, issued together.  The row loads wait for neither LDS nor a barrier: the barrier
//    that publishes the packed pair gradients comes behind their issue;
//  - the pair gradients (the MFMA A operands) are read from LDS without a branch (clamped index, select), all
//    of them before the first MFMA, so the MFMAs of a step issue back to back;
//  - per column step s in ascending order: wait for its row, write its tile row, its MFMAs -- the MFMAs track
//    the arrivals;
//  - tile row 0 (features 0..15) is accumulated over every step first and stored, then tile row 1: row 0's stores
//    drain while row 1's MFMAs run on rows that have landed.
// Every accumulator sums its steps in ascending order, as in the kernel's text: dx, dt and the table rows keep
// every bit.  Bounds behaviour, zero rows for invalid indices and `frozen` are the kernel's.
template <int NB, int SPB>
__device__ __forceinline__ void bwd_split_tracked(int F, int B, const float* __restrict__ dout, int64_t dout_ld,
                                                  float* __restrict__ dx, int64_t dx_ld, float* __restrict__ dt,
                                                  int64_t dt_ld, const GatherArgs& ga, const float* __restrict__ x,
                                                  int64_t x_ld, const StepUpdate& su) {
    constexpr int NS = 16 * NB, KS = 4 * NB, PMAX = NS * (NS - 1) / 2, d = 128;
    __shared__ float pk_all[SPB][PMAX];                                      // each sample's packed gradient row
    __shared__ __attribute__((aligned(16))) float tt_all[2 * SPB][NS * 64];  // each wave's tile of T
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pair = w >> 1, h = w & 1;
    const int c = lane & 15, q = lane >> 4;
    const int64_t b = (int64_t)blockIdx.x * SPB + pair;
    const bool live = b < B;
    const int64_t bb = live ? b : 0;  // a padding sample reads sample 0 (and stores nothing)
    const int ksteps = (F + 3) / 4;
    const int P = F * (F - 1) / 2;
    const float* ob = dout + bb * dout_ld;
    float* pk = pk_all[pair];
    float* Tt = tt_all[w];
    const int n0 = 64 * h + 4 * c;  // this lane's 4 output columns
#ifdef DLRM_WTRACE
    unsigned long long wts_[7] = {0, 0, 0, 0, 0, 0, 0};
#endif
    WTS(0);
    // ---- every independent load first: table `lane`'s descriptor, index and flag, the packed gradients, x part
    const bool tl = lane < F - 1;
    const TableDesc tdl = load_table(ga.tabs, tl ? lane : 0);
    const int64_t myidx = load_index_if(tl, ga.idx, ga.itype, (int64_t)(tl ? lane : 0) * ga.tstride + bb);
    // (su.single NULL: no once-hit update, every table row goes to dt; the load executes either way, so no branch
    // joins behind it with a wait for every load before it)
    const uint8_t* flp = su.single ? su.single + (tl ? (int64_t)lane * su.cap + bb : 0) : (const uint8_t*)ga.tabs;
    const uint8_t myfl0 = ldg<uint8_t>(flp);
    const uint8_t myfl = su.single ? myfl0 : (uint8_t)0;
    constexpr int PPW = (PMAX + 127) / 128;  // packed values staged per lane
    float pv[PPW];
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
        const int p = h * 64 + lane + 128 * k;
        pv[k] = ldg<float>(ob + d + (p < P ? p : 0));  // (masked where it is staged: no wait for it before the rows)
    }
    const f32x4_t xo = load4_f32(ob + n0);  // dout's x part at this lane's columns (lanes 0..15 hold output row 0)
    const bool frozen = su.single ? *su.err != 0 : true;  // a bounds error this step: no table row is written
    // ---- this lane's row: validated here, its address (0: invalid / no table) and its address as a once-hit row
    const int64_t myr = myidx - ga.base;
    const bool myok = tl && myr >= 0 && myr < tdl.nrows;
    if (tl && !myok && h == 0 && live) raise_index_error(ga.err);
    const long long myad = myok ? (long long)tdl.data + myr * (int64_t)(d * sizeof(float)) : 0ll;
    const long long myua = (myfl != 0 && !frozen) ? myad : 0ll;
    WTS_USE(myad);
    WTS(1);
    const float* rowp[KS];
    unsigned livek = 0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int kk = 4 * s + q;  // (kk >= F: lane kk - 1 holds no table, its address is 0)
        const long long a = __shfl(myad, kk >= 1 ? kk - 1 : 0, 64);
        const float* src = kk == 0 ? x + bb * x_ld : (const float*)a;
        livek |= src ? (1u << s) : 0u;
        rowp[s] = src ? src : ob;
    }
    // the row loads in step order (the steps' waits count on it), every address formed before the first
    __builtin_amdgcn_sched_barrier(0);
    f32x4_t bv[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        bv[s] = load4_f32(rowp[s] + n0);
        __builtin_amdgcn_sched_barrier(0);
        if (s == 0) WTS(2);
    }
    // ---- behind the row loads' issue: the packed gradients to LDS, the block's barrier, the A operands
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
        const int p = h * 64 + lane + 128 * k;
        if (p < PMAX) pk[p] = p < P ? pv[k] : 0.0f;
    }
    __syncthreads();  // pk
    float av[KS][NB];  // S[16I+c][4s+q]: the symmetric zero-diagonal unpack of the pair row
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int I = 0; I < NB; ++I) {
            const int i = I * 16 + c, kk = 4 * s + q;
            const int hi = i > kk ? i : kk, lo = i > kk ? kk : i;
            const bool on = i != kk && hi < F;
            const float v = pk[on ? hi * (hi - 1) / 2 + lo : 0];
            av[s][I] = on ? v : 0.0f;
        }
    f32x4_t acc[NB][4];
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[I][e] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_sched_barrier(0);
    // step s's row has landed: its tile row (the once-hit update reads the tile)
    auto land = [&](int s) {
        bv[s] = ((livek >> s) & 1u) ? bv[s] : f32x4_t{0.f, 0.f, 0.f, 0.f};
        *(f32x4_t*)(Tt + (4 * s + q) * 64 + 4 * c) = bv[s];
    };
    auto mfma = [&](int s, int I) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            acc[I][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s][I], bv[s][e], acc[I][e], 0, 0, 0);
    };
    // tile row I's four output rows per lane, f = 16I + 4q + r: the table row itself when once-hit, else its dt row
    // (the training step (su.single set) leaves dt's x row alone: dx carries it)
    auto store = [&](int I) {
        long long ua[4];
        f32x4_t tw[4];  // the rows as gathered
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = I * 16 + 4 * q + r;  // (f >= F: lane f - 1 holds no table)
            const long long a = __shfl(myua, f >= 1 ? f - 1 : 0, 64);
            ua[r] = f >= 1 ? a : 0ll;
            tw[r] = *(const f32x4_t*)(Tt + f * 64 + 4 * c);
        }
        if (!live) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = I * 16 + 4 * q + r;
            if (f < F) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[I][e][r];
                if (ua[r]) {
                    float wv[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) wv[e] = __builtin_fmaf(-su.lr, 0.0f + v[e], tw[r][e]);
                    store_row<float, 4, true>((float*)ua[r], n0, wv);
                } else if (f > 0 || !su.single) {
                    stg_nt<f32x4_t>(dt + b * dt_ld + (int64_t)f * d + n0, f32x4_t{v[0], v[1], v[2], v[3]});
                }
                if (f == 0)
                    stg<f32x4_t>(dx + b * dx_ld + n0,
                                 f32x4_t{xo[0] + v[0], xo[1] + v[1], xo[2] + v[2], xo[3] + v[3]});
            }
        }
    };
    // tile row 0 (features 0..15) over every step first, then its stores, which drain under tile row 1's MFMAs
    // (on landed rows), then tile row 1's stores
#pragma unroll
    for (int I = 0; I < NB; ++I) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            if (s < ksteps) {
                if (I == 0) {
                    if (s == 0 || s == ksteps - 1) WTS_USE(bv[s]);
                    if (s == 0) WTS(3);
                    if (s == ksteps - 1) WTS(4);
                    land(s);
                }
                mfma(s, I);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (I == 0) wave_lds_sync();  // the tile of T
        if (I == NB - 1) {
            WTS_USE(acc[I][3]);
            WTS(5);
        }
        store(I);
        __builtin_amdgcn_sched_barrier(0);
    }
    WTS(6);
    if (h == 0) BWTS_FLUSH(b);
    // (a flat store: behind the last wait on a load, so that every such wait keeps its count)
    if (su.single && blockIdx.x == 0 && threadIdx.x == 0) snapshot_error(su.err, frozen ? 1u : 0u);
}

// The training step's backward with each sample split over TWO waves by column halves (wave h
// takes the 64-column super-blocks sb = h, h + 2, ...): every wave's dependent chain (indices ->
// rows -> MFMA -> stores) is half as long and needs about half the registers, so four waves per
// SIMD stay resident (B = 2048: all 4096 waves at once) instead of two.  The math per
// super-block is bwd_body's MFMA sequence, so dx, dt and the tables are bit-identical to
// interact_bwd_update_kernel's.
// This path is bound by the vector-memory INSTRUCTION rate of a CU as much as by bytes, so a wave
// issues few loads:
//  - lane t < T loads table t's index and once-hit flag for the sample (one instruction each),
//    validates it and shuffles the row to the lanes that need it (ds_bpermute, not the TA);
//  - the packed pair gradients dout[b][d : d + P] are staged in LDS by the pair's two waves
//    with contiguous loads, and the MFMA A operand S[i][j] is read from there by pair index (no
//    S matrix, no scatter);
//  - dout's x part (dx = dout_x + dt row 0) is one coalesced load of the wave's 64 columns,
//    redistributed by shuffles;
//  - a once-hit row's old value comes from the gathered rows, moved from the B-operand layout
//    (lane (c, q): row 4s + q) to the accumulator layout (row 16I + 4q + r) through the wave's
//    LDS tile, not re-read from HBM.
// One block = SPB samples (WPS·SPB waves; grid = ceil(B / SPB)), one pass: both barriers are
// reached by every wave.  Larger blocks shorten the dispatch ramp (fewer workgroups to place).
// WPS = 1 (d <= 64, one super-block): one wave per sample, the same per-sample load plan --
// the bwd_body kernel's per-lane index / flag loads (KS + 8 NB instructions before the rows)
// are most of a small-d backward's time.
// MAPPED (dlrm_interact_bwd_blocked): table rows' gradients go to the send layout (GatherArgs dtb /
// dtl), none to dt's x row; a separate instantiation, so the step kernels keep their LDS budget.
// CPL = 8 (bf16 rows): a lane loads 8 columns (16 B) of each row and runs 8 MFMAs per k-step, so
// a super-block is 128 columns and one wave takes a d = 128 sample whole (half the load
// instructions per byte of the 4-column form, and more samples resident per CU); the gathered
// rows stay bf16 in the wave's LDS tile.  Every output element is the same MFMA sum over the same
// k-steps as in the 4-column form: dx, dt and the tables are bit-identical.
// YS (dlrm_interact_bwd on a materialized ys, e.g. pooled bags): T row kk of sample b is ys row
// x + b * x_ld + kk * d (x / x_ld carry ys / ys_ld), no index, flag or once-hit update; every dt row
// is written.  Up to 96 features (NB <= 6): the gather-free backward of the pooled workload
// (F = 65), one wave per 64-column super-block.
// SU: the once-hit rule and its arguments.  StepUpdate is Descent's write.  SplitStepUpdate (dlrm_split_step_bwd) is
// the split rule's on bf16 tables, its branches `if constexpr (SU::kSplit)`; AdagradStepUpdate (dlrm_adagrad_step_bwd)
// the sparse Adagrad rules' on fp32 and bf16 tables, `if constexpr (AG == 1)` the element-wise rule and `(AG == 2)`
// the row-wise one; StochasticStepUpdate (dlrm_sr_step_bwd) the stochastic rule's on bf16 tables, `if constexpr
// (SU::kStochastic)`: Descent's write with the rule's store; StochasticAdagradStepUpdate (dlrm_sr_adagrad_step_bwd) the
// seeded Adagrad rules' on bf16 tables: the `AG` branches, ending in SrWord's store.
// The rules other than Descent exist in the step's
// default geometries only, NB = 1 and 2
// (step_bwd_form below).  (The body stays the kernel's own text: as an inlined function template it no longer
// compiled to the same code.)
template <typename T, int NB, int DC, int SPB, int WPS = 2, bool MAPPED = false, int CPL = 4, bool YS = false,
          typename SU = StepUpdate>
__global__ __launch_bounds__(64 * WPS * SPB, CPL == 8 ? 3 : (NB > 2 ? 2 : 4)) void interact_bwd_split_kernel(
    int d_, int F, int B, const T* __restrict__ dout, int64_t dout_ld, float* __restrict__ dx, int64_t dx_ld,
    float* __restrict__ dt, int64_t dt_ld, GatherArgs ga, const T* __restrict__ x, int64_t x_ld, SU su) {
    static_assert(CPL == 4 || (CPL == 8 && sizeof(T) == 2), "8 columns per lane: bf16 rows");
    static_assert(!SU::kSplit || (sizeof(T) == 2 && !YS && !MAPPED), "split rows live in bf16 tables");
    constexpr int AG = SU::kAdagrad;
    constexpr bool RULE = SU::kSplit || AG != 0;  // a rule whose rows have a second stream
    typedef typename SU::State SE;
    static_assert(AG == 0 || (!YS && !MAPPED), "the Adagrad rules step the training step's tables");
    static_assert(!SU::kStochastic || (sizeof(T) == 2 && !YS && !MAPPED), "stochastic rounding is of bf16 tables");
    // the row-wise sum of squares crosses the sample's two waves once: one super-block per wave, so the block
    // barrier of that exchange sits in uniform control flow
    static_assert(AG != 2 || WPS == 1 || DC == 128, "row-wise over two waves: d = 128");
    if constexpr (bwd_tracked<T, DC, WPS, MAPPED, CPL, YS, SU>()) {
        bwd_split_tracked<NB, SPB>(F, B, dout, dout_ld, dx, dx_ld, dt, dt_ld, ga, x, x_ld, su);
        return;
    }
    constexpr int NS = 16 * NB;
    constexpr int KS = 4 * NB;
    constexpr int PMAX = NS * (NS - 1) / 2;
    constexpr int SBC = 16 * CPL;  // columns per super-block
    // the wave's tile of T: fp32 (CPL = 4) or the rows' own bf16 (CPL = 8)
    typedef typename std::conditional<CPL == 8, uint16_t, float>::type TileT;
    const int d = DC > 0 ? DC : d_;
    __shared__ float pk_all[SPB][PMAX];  // each sample's packed gradient row
    // each wave's tile of T (the once-hit update reads it; YS has none)
    __shared__ __attribute__((aligned(16))) TileT tt_all[YS ? 1 : WPS * SPB][YS ? 4 : NS * SBC];
    __shared__ TableDesc tds[YS ? 1 : NS];
    __shared__ int64_t dmap[MAPPED ? 2 * NS : 1];  // table t's dt rows at dt + dmap[t] + b * dmap[F - 1 + t]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pair = w / WPS, h = w % WPS;
    constexpr bool mapped = MAPPED;
    const int c = lane & 15, q = lane >> 4;
    const int64_t b = (int64_t)blockIdx.x * SPB + pair;
    const bool live = b < B;
    const int64_t bb = live ? b : 0;  // a padding sample reads sample 0 (and stores nothing)
    const int ksteps = (F + 3) / 4;
    const int P = F * (F - 1) / 2;
    const T* ob = dout + bb * dout_ld;
    float* pk = pk_all[pair];
    TileT* Tt = tt_all[YS ? 0 : w];
    if (h == 0) WT(1, 0, b);
    // the table descriptors (F - 1 <= NS <= 32 < blockDim: one per thread), held in registers and
    // written to LDS after the other independent loads are issued, so no wave waits for them alone
    const bool tdl_ok = !YS && (int)threadIdx.x < F - 1;
    const TableDesc tdl = YS ? TableDesc{nullptr, 0} : load_table(ga.tabs, tdl_ok ? (int)threadIdx.x : 0);
    int64_t dm0 = 0, dm1 = 0;
    if constexpr (MAPPED) {
        dm0 = ldg<int64_t>(ga.dtb + (tdl_ok ? threadIdx.x : 0));
        dm1 = ldg<int64_t>(ga.dtl + (tdl_ok ? threadIdx.x : 0));
    }
    // ---- every independent load first: table `lane`'s index and flag, the packed gradients, x part
    const bool tl = !YS && lane < F - 1;
    const int64_t myidx = YS ? 0 : load_index_if(tl, ga.idx, ga.itype, (int64_t)(tl ? lane : 0) * ga.tstride + bb);
    // su.single NULL (dlrm_interact_bwd_blocked, YS): no once-hit update, every table row goes to dt
    const uint8_t myfl = su.single ? ldg<uint8_t>(su.single + (tl ? (int64_t)lane * su.cap + bb : 0)) : (uint8_t)0;
    // split, Adagrad: the tables' pointers to the low halves / the state reach the writing lanes through LDS, beside
    // tds (d = 128: the forms with 256 B of LDS to spare at their occupancy), else as the rows do, by shuffle
    // from lane t
    constexpr bool ST_LDS = DC == 128;
    long long myst = 0;
    SE** sop = nullptr;
    if constexpr (RULE) {
        if constexpr (ST_LDS) {
            sop = rule_tab<SE, NS>();
            myst = (long long)ldg<SE*>(rule_state(su) + (tdl_ok ? threadIdx.x : 0));
        } else {
            myst = (long long)ldg<SE*>(rule_state(su) + (tl ? lane : 0));
        }
    }
    constexpr int PPW = (PMAX + 64 * WPS - 1) / (64 * WPS);  // packed values staged per lane
    float pv[PPW];
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
        const int p = h * 64 + lane + 64 * WPS * k;
        const float v = to_f32(ldg<T>(ob + d + (p < P ? p : 0)));
        pv[k] = p < P ? v : 0.0f;
    }
    // super-blocks per wave (CPL = 4, WPS = 2: d <= 512 when not fixed; WPS = 1: d <= 64;
    // CPL = 8: d <= 128, one wave)
    // (DC = 0: WPS = 1 / 2 cover d <= 64 / 512; YS: d = 64 * WPS, one super-block per wave)
    constexpr int SBW = YS ? 1
                           : DC > 0 ? ((DC / SBC + WPS - 1) / WPS > 0 ? (DC / SBC + WPS - 1) / WPS : 1)
                                    : (WPS == 2 ? 4 : 1);
    constexpr int XV = SBC / 64;  // dout x-part values per lane and super-block
    float xv[SBW][XV];
#pragma unroll
    for (int sbi = 0; sbi < SBW; ++sbi)
#pragma unroll
        for (int k = 0; k < XV; ++k) {
            const int n = SBC * h + SBC * WPS * sbi + 64 * k + lane;
            xv[sbi][k] = to_f32(ldg<T>(ob + (n < d ? n : 0)));
        }
    const bool frozen = su.single ? *su.err != 0 : true;  // a bounds error this step: no table row is written
    if (su.single && blockIdx.x == 0 && threadIdx.x == 0) snapshot_error(su.err, frozen ? 1u : 0u);
    // the stochastic rule with the step word's value: read once per workgroup, into two scalars
    StochasticDescent sr{};
    SrWord sw{};  // (the seeded Adagrad rules: the same word, their store)
    if constexpr (SU::kStochastic && AG == 0) {
        sr = StochasticDescent{su.lr, su.k0, su.k1, su.step, 0u, 0u};
        sr.load_step();
    } else if constexpr (SU::kStochastic) {
        sw = SrWord{su.k0, su.k1, su.step, 0u, 0u};
        sw.load_step();
    }
    if (tdl_ok) {
        tds[threadIdx.x] = tdl;
        if constexpr (RULE && ST_LDS) sop[threadIdx.x] = (SE*)myst;
        if constexpr (MAPPED) {
            dmap[threadIdx.x] = dm0;
            dmap[F - 1 + threadIdx.x] = dm1;
        }
    }
#pragma unroll
    for (int k = 0; k < PPW; ++k) {
        const int p = h * 64 + lane + 64 * WPS * k;
        if (p < PMAX) pk[p] = pv[k];
    }
    __syncthreads();  // tds, pk
    // validate this lane's table index; rows travel as 32-bit (~0u = invalid / no table)
    uint32_t myrow = ~0u;
    if (tl) {
        const int64_t r = myidx - ga.base;
        if (r >= 0 && r < tds[lane].nrows) myrow = (uint32_t)r;
        else if (h == 0 && live) raise_index_error(ga.err);
    }
    const T* rowp[KS];
    unsigned livek = 0;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int kk = 4 * s + q;
        const uint32_t r = (uint32_t)__shfl((int)myrow, kk >= 1 ? kk - 1 : 0, 64);
        const bool tab = s < ksteps && kk >= 1 && kk < F && r != ~0u;
        const T* src = YS ? ((s < ksteps && kk < F) ? x + bb * x_ld + (int64_t)kk * d : nullptr)
                   : (s < ksteps && kk == 0) ? x + bb * x_ld
                                             : (tab ? (const T*)tds[kk - 1].data + (int64_t)r * d : nullptr);
        livek |= src ? (1u << s) : 0u;
        // (CPL = 8: a masked row reads the zero row -- a 16-B aligned source whatever dout's layout)
        rowp[s] = src ? src : (CPL == 8 ? (const T*)g_zero_row : ob);
    }
    uint32_t urow[NB][4];
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = I * 16 + 4 * q + r;
            const int src = (f >= 1 && f < F) ? f - 1 : 0;
            const uint32_t row = (uint32_t)__shfl((int)myrow, src, 64);
            const int fl = __shfl((int)myfl, src, 64);
            urow[I][r] = (f >= 1 && f < F && !frozen && fl != 0) ? row : ~0u;
        }
    if (h == 0) WT(1, 1, b);
#pragma unroll
    for (int sbi = 0; sbi < SBW; ++sbi) {
        const int sb = SBC * h + SBC * WPS * sbi;
        if (sb >= d) break;
        const int n0 = sb + CPL * c;  // this lane's CPL output columns
        const bool colok = n0 < d;
        const int nc = colok ? n0 : 0;
        f32x4_t acc[NB][CPL];
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int e = 0; e < CPL; ++e) acc[I][e] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if constexpr (CPL == 4) {
            f32x4_t bv[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const f32x4_t v = load4_f32(rowp[s] + nc);
                bv[s] = ((livek >> s) & 1u) && colok ? v : f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
            if (sbi > 0) wave_lds_sync();  // the previous super-block's tile reads are done
#pragma unroll
            for (int s = 0; s < KS; ++s)
                if (s < ksteps) *(f32x4_t*)(Tt + (4 * s + q) * SBC + 4 * c) = bv[s];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if (s < ksteps) {
                    const int kk = 4 * s + q;
#pragma unroll
                    for (int I = 0; I < NB; ++I) {
                        // S[16I+c][kk]: the symmetric zero-diagonal unpack of the pair row
                        const int i = I * 16 + c;
                        const int hi = i > kk ? i : kk, lo = i > kk ? kk : i;
                        const float av = (i != kk && hi < F) ? pk[hi * (hi - 1) / 2 + lo] : 0.0f;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            acc[I][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[s][e], acc[I][e], 0, 0, 0);
                    }
                }
            }
        } else {
            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
            u32x4_t bv[KS];  // 8 bf16 columns of row 4s+q, packed
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const u32x4_t v = ldg<u32x4_t>(rowp[s] + nc);
                bv[s] = ((livek >> s) & 1u) && colok ? v : u32x4_t{0u, 0u, 0u, 0u};
            }
            if (sbi > 0) wave_lds_sync();  // the previous super-block's tile reads are done
#pragma unroll
            for (int s = 0; s < KS; ++s)
                if (s < ksteps) *(u32x4_t*)(Tt + (4 * s + q) * SBC + 8 * c) = bv[s];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                if (s < ksteps) {
                    const int kk = 4 * s + q;
#pragma unroll
                    for (int I = 0; I < NB; ++I) {
                        const int i = I * 16 + c;
                        const int hi = i > kk ? i : kk, lo = i > kk ? kk : i;
                        const float av = (i != kk && hi < F) ? pk[hi * (hi - 1) / 2 + lo] : 0.0f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const uint32_t wd = bv[s][e >> 1];
                            const float bvf = __uint_as_float((e & 1) ? (wd & 0xffff0000u) : (wd << 16));
                            acc[I][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bvf, acc[I][e], 0, 0, 0);
                        }
                    }
                }
            }
        }
        if (h == 0 && sbi == 0) WT(1, 2, b);
        // dout's x part for this lane's columns (lanes 0..15 hold output row 0)
        float xo[CPL];
#pragma unroll
        for (int e = 0; e < CPL; ++e) {
            const int n = CPL * c + e;  // column within the super-block: lane n & 63 of xv[sbi][n >> 6]
            float xs = __shfl(xv[sbi][0], n & 63, 64);
#pragma unroll
            for (int k = 1; k < XV; ++k) {
                const float t = __shfl(xv[sbi][k], n & 63, 64);
                xs = (n >> 6) == k ? t : xs;
            }
            xo[e] = xs;
        }
        wave_lds_sync();  // the tile of T (written before the MFMAs)
        // split, element-wise Adagrad: pointers by shuffle here, in uniform control flow and after the MFMAs (held
        // through them, with the gathered rows in flight, they cost the one-wave form registers it does not have
        // at 32 features)
        SE* ust[NB][4];
        if constexpr ((SU::kSplit || AG == 1) && !ST_LDS) {
#pragma unroll
            for (int I = 0; I < NB; ++I)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = I * 16 + 4 * q + r;
                    ust[I][r] = (SE*)__shfl(myst, (f >= 1 && f < F) ? f - 1 : 0, 64);
                }
        }
        // (row-wise: its shuffles and its block barrier need uniform control flow, so padding samples and lanes
        // past the row come along into the loop and leave it per tile row, after the row sums)
        if constexpr (AG != 2) {
            if (!live || !colok) continue;
        }
#pragma unroll
        for (int I = 0; I < NB; ++I) {
            // the second stream of the four rows of tile row I: each one's table pointer (st_base; by shuffle: usr,
            // which the row-wise rule fills below) and the lane's CPL columns of its row (st_row)
            SE* usr[4];
            if constexpr ((SU::kSplit || AG == 1) && !ST_LDS) {
#pragma unroll
                for (int r = 0; r < 4; ++r) usr[r] = ust[I][r];
            }
            auto st_base = [&](int r) {
                const int f = I * 16 + 4 * q + r;
                SE* base;
                if constexpr (ST_LDS) base = sop[f - 1];
                else base = usr[r];
                return base;
            };
            auto st_row = [&](auto r) { return st_base(r) + (int64_t)urow[I][r] * d + n0; };  // (generic: State may be void)
            // split: the low halves of this lane's once-hit rows among the four of tile row I (its CPL columns),
            // loaded together before the first of them is written (8 columns per lane: each at its write --
            // four 16-B vectors would take that form from 6 to 4 waves per SIMD at 16 features).  Issued
            // behind the gathered rows they would travel beside the gather, but waiting as bits through the
            // MFMAs they took the two-wave form from 8 to 6 waves per SIMD at 16 features and spilt at 32.
            typename Halves<CPL>::type lov[4];
            if constexpr (SU::kSplit && CPL == 4) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (I * 16 + 4 * q + r < F && urow[I][r] != ~0u) lov[r] = load_halves<CPL>(st_row(r));
            }
            // Adagrad: the state of this lane's once-hit rows, loaded here as the low halves are (after the
            // MFMAs, the four of a tile row together) -- the element-wise rule's fp32 state row at the lane's
            // columns (8 columns per lane: each at its write), the row-wise rule's word
            // (with up to 16 features the state is loaded at each row's write instead: four in flight took the
            // NB = 1 forms below Descent's 8 waves per SIMD)
            // (the seeded row-wise rule's one-wave form too: four words in flight beside the Philox rounds spilt 3
            // registers at its 128)
            constexpr bool ST4 = NB > 1 && CPL == 4 && !(SU::kStochastic && AG == 2 && WPS == 1);
            // row-wise: the four tile rows' sums of squares of G = 0 + g, in the order of the apply's once-hit item
            // (apply.hpp run_singles, fp32 gradient rows: apply lane v holds columns 4v..4v+3) -- a lane's fma
            // chain from 0 over four columns in column order, then the xor butterfly over the row's lanes from
            // distance 1 up.  Lane c holds apply lane 16h + c's columns (8 columns per lane: lanes 2c and 2c + 1,
            // so its two chains' sum is level 1 and the butterfly over c levels 2..16); a lane past the row
            // (!colok: its accumulators are 0) adds +0, which keeps the bits of a sum >= 0.  d = 128 over two
            // waves: each wave's 64 columns over c, then the last level, one commutative add of the two waves'
            // totals, through LDS (a slot per tile row I: one barrier each, nothing is overwritten).
            // The state word m of a row is one address for both waves, and wave 0 stores m' there: so only wave 0
            // ever loads it (its c == 0 lanes, before the barrier) and hands it to both waves through the same LDS
            // exchange.  Wave 1 never reads a word that wave 0 writes.
            float rs[4];
            float mx[4];  // two waves: the rows' state words, out of LDS
            if constexpr (AG == 2) {
                float m0w[4];
                if constexpr (WPS == 2) {
                    if (h == 0 && c == 0 && live) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int f = I * 16 + 4 * q + r;
                            if (f < F && urow[I][r] != ~0u) m0w[r] = ldg<float>(sop[f - 1] + urow[I][r]);
                        }
                    }
                }
                if constexpr (!ST_LDS) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = I * 16 + 4 * q + r;
                        usr[r] = (SE*)__shfl(myst, (f >= 1 && f < F) ? f - 1 : 0, 64);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float g[CPL];
#pragma unroll
                    for (int e = 0; e < CPL; ++e) g[e] = 0.0f + acc[I][e][r];
                    float ss = sum_squares<4>(g, 0.0f);
                    if constexpr (CPL == 8) ss += sum_squares<4>(g + 4, 0.0f);
#pragma unroll
                    for (int o = 1; o < 16; o <<= 1) ss += __shfl_xor(ss, o, 64);
                    rs[r] = ss;
                }
                if constexpr (WPS == 2) {
                    float* sx = row_ss_tab<SPB * 3 * NS>();  // [SPB][wave 0's sums, wave 1's sums, m][NS]
                    if (c == 0) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) sx[(pair * 3 + h) * NS + I * 16 + 4 * q + r] = rs[r];
                        if (h == 0 && live) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int f = I * 16 + 4 * q + r;
                                if (f < F && urow[I][r] != ~0u) sx[(pair * 3 + 2) * NS + f] = m0w[r];
                            }
                        }
                    }
                    __syncthreads();
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        rs[r] += sx[(pair * 3 + (h ^ 1)) * NS + I * 16 + 4 * q + r];
                        mx[r] = sx[(pair * 3 + 2) * NS + I * 16 + 4 * q + r];
                    }
                }
                if (!live || !colok) continue;
            }
            f32x4_t sv[AG == 1 && ST4 ? 4 : 1];
            float mv[AG == 2 && ST4 && WPS == 1 ? 4 : 1];
            if constexpr (AG == 1 && ST4) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (I * 16 + 4 * q + r < F && urow[I][r] != ~0u)
                        sv[r] = ldg<f32x4_t>(st_row(r));
            }
            if constexpr (AG == 2 && ST4 && WPS == 1) {  // (one wave holds the row: its own loads, then its store)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (I * 16 + 4 * q + r < F && urow[I][r] != ~0u) mv[r] = ldg<float>(st_base(r) + urow[I][r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = I * 16 + 4 * q + r;
                if (f < F) {
                    float v[CPL];
#pragma unroll
                    for (int e = 0; e < CPL; ++e) v[e] = acc[I][e][r];
                    if (urow[I][r] != ~0u) {
                        float wv[CPL];
                        float tw[CPL];  // the row as gathered
                        if constexpr (CPL == 4) {
                            const f32x4_t t4 = *(const f32x4_t*)(Tt + f * SBC + 4 * c);
#pragma unroll
                            for (int e = 0; e < 4; ++e) tw[e] = t4[e];
                        } else {
                            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
                            const u32x4_t t8 = *(const u32x4_t*)(Tt + f * SBC + 8 * c);
#pragma unroll
                            for (int e = 0; e < 8; ++e)
                                tw[e] = __uint_as_float((e & 1) ? (t8[e >> 1] & 0xffff0000u) : (t8[e >> 1] << 16));
                        }
                        if constexpr (SU::kSplit) {
                            // (either tile layout gives the element's bf16 bits << 16 exactly)
                            const int64_t ro = (int64_t)urow[I][r] * d + n0;
                            uint32_t hb[CPL];
#pragma unroll
                            for (int e = 0; e < CPL; ++e) hb[e] = __float_as_uint(tw[e]);
                            if constexpr (CPL == 8) lov[r] = load_halves<CPL>(st_row(r));
                            split_once_hit<CPL>(su.lr, v, hb, lov[r], (uint16_t*)tds[f - 1].data + ro, st_row(r));
                        } else if constexpr (AG == 1) {
                            // A += G^2, w -= lr G / (sqrt(A) + eps) with G = 0 + g: apply.hpp's adagrad_step
                            float* srow = st_row(r);
                            float gg[CPL], av[CPL];
#pragma unroll
                            for (int e = 0; e < CPL; e += 4) {
                                f32x4_t a4;
                                if constexpr (ST4) a4 = sv[r];
                                else a4 = ldg<f32x4_t>(srow + e);
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    av[e + k] = a4[k];
                                    gg[e + k] = 0.0f + v[e + k];
                                }
                            }
                            adagrad_step<CPL>(su.lr, su.eps, gg, av, tw);
#pragma unroll
                            for (int e = 0; e < CPL; e += 4)
                                stg_nt<f32x4_t>(srow + e, f32x4_t{av[e], av[e + 1], av[e + 2], av[e + 3]});
                            if constexpr (SU::kStochastic)  // (W' as the parent makes it, the rule's store)
                                sw.template store<CPL>((uint16_t*)tds[f - 1].data + (int64_t)urow[I][r] * d + n0, f - 1,
                                                       urow[I][r], n0, tw);
                            else
                            store_row<T, CPL, true>((T*)tds[f - 1].data + (int64_t)urow[I][r] * d, n0, tw);
                        } else if constexpr (AG == 2) {
                            // m += ss / D, w -= (lr / (sqrt(m) + eps)) G: apply.hpp's helpers, one lane stores m
                            float m0;
                            if constexpr (WPS == 2) m0 = mx[r];
                            else if constexpr (ST4) m0 = mv[r];
                            else m0 = ldg<float>(st_base(r) + urow[I][r]);
                            const float m = rowwise_m(m0, rs[r], d);
                            const float sc = rowwise_scale(su.lr, su.eps, m);
#pragma unroll
                            for (int e = 0; e < CPL; ++e) wv[e] = __builtin_fmaf(-sc, 0.0f + v[e], tw[e]);
                            if constexpr (SU::kStochastic)
                                sw.template store<CPL>((uint16_t*)tds[f - 1].data + (int64_t)urow[I][r] * d + n0, f - 1,
                                                       urow[I][r], n0, wv);
                            else
                            store_row<T, CPL, true>((T*)tds[f - 1].data + (int64_t)urow[I][r] * d, n0, wv);
                            if (c == 0 && h == 0) stg<float>(st_base(r) + urow[I][r], m);
                        } else if constexpr (SU::kStochastic) {
                            // Descent's step, stored by the apply's own store: one Philox block per four columns
                            // from column n0 of row urow of table f - 1
#pragma unroll
                            for (int e = 0; e < CPL; ++e) wv[e] = __builtin_fmaf(-su.lr, 0.0f + v[e], tw[e]);
                            sr.template store<CPL>((uint16_t*)tds[f - 1].data + (int64_t)urow[I][r] * d + n0, f - 1,
                                                   urow[I][r], n0, wv);
                        } else {
#pragma unroll
                        for (int e = 0; e < CPL; ++e) wv[e] = __builtin_fmaf(-su.lr, 0.0f + v[e], tw[e]);
                        store_row<T, CPL, true>((T*)tds[f - 1].data + (int64_t)urow[I][r] * d, n0, wv);
                        }
                    } else if (!mapped && (f > 0 || !su.single)) {
                        // (the training step (su.single set) leaves dt's x row alone: dx carries it)
                        // (CPL = 8: a lane's two 16-B pieces are 32 B apart, so each store instruction
                        // covers half of every line: plain stores let L2 merge the halves, where
                        // non-temporal ones left as partial-line writes, 95 -> 117 MB per launch)
#pragma unroll
                        for (int e = 0; e < CPL; e += 4) {
                            const f32x4_t pv4 = f32x4_t{v[e], v[e + 1], v[e + 2], v[e + 3]};
                            if constexpr (CPL == 8) stg<f32x4_t>(dt + b * dt_ld + (int64_t)f * d + n0 + e, pv4);
                            else stg_nt<f32x4_t>(dt + b * dt_ld + (int64_t)f * d + n0 + e, pv4);
                        }
                    } else if (f > 0) {
#pragma unroll
                        for (int e = 0; e < CPL; e += 4)
                            stg_nt<f32x4_t>(dt + dmap[f - 1] + b * dmap[F - 2 + f] + n0 + e,
                                            f32x4_t{v[e], v[e + 1], v[e + 2], v[e + 3]});
                    }
                    if (f == 0)
#pragma unroll
                        for (int e = 0; e < CPL; e += 4)
                            stg<f32x4_t>(dx + b * dx_ld + n0 + e, f32x4_t{xo[e] + v[e], xo[e + 1] + v[e + 1],
                                                                         xo[e + 2] + v[e + 2], xo[e + 3] + v[e + 3]});
                }
            }
        }
        if (h == 0 && sbi == 0) {
            WT(1, 3, b);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            WT(1, 4, b);
        }
    }
}

// ------------------------------------------------------------------ scalar fallbacks
template <typename T>
__global__ __launch_bounds__(256) void interact_fwd_scalar(int d, int F, int B, const T* __restrict__ x, int64_t x_ld,
                                                           T* __restrict__ ys, int64_t ys_ld, T* __restrict__ out,
                                                           int64_t out_ld, int padding) {
    const int P = F * (F - 1) / 2;
    const int W = d + P + padding;
    const int64_t total = (int64_t)B * W;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = e / W;
        const int k = (int)(e % W);
        const T* xb = x + b * x_ld;
        if (k < d) {
            ys[b * ys_ld + k] = xb[k];
            out[b * out_ld + k] = xb[k];
        } else if (k < d + P) {
            const int p = k - d;
            int i = 1;
            while ((i + 1) * i / 2 <= p) ++i;
            const int j = p - i * (i - 1) / 2;
            const T* ri = i == 0 ? xb : ys + b * ys_ld + (int64_t)i * d;
            const T* rj = j == 0 ? xb : ys + b * ys_ld + (int64_t)j * d;
            float z = 0.0f;
            for (int cc = 0; cc < d; ++cc) z = fmaf(to_f32(ri[cc]), to_f32(rj[cc]), z);
            out[b * out_ld + k] = from_f32<T>(z);
        } else {
            out[b * out_ld + k] = from_f32<T>(0.0f);
        }
    }
}

template <typename T, bool GATHER>
__device__ __forceinline__ float t_elem(const T* t, int64_t t_ld, int64_t b, int j, int n, int d, const GatherArgs& ga,
                                        const T* x, int64_t x_ld) {
    if (!GATHER) return to_f32(t[b * t_ld + (int64_t)j * d + n]);
    if (j == 0) return to_f32(x[b * x_ld + n]);
    const int64_t r = load_index(ga.idx, ga.itype, (j - 1) * ga.tstride + b * ga.L) - ga.base;
    if (r < 0 || r >= ga.tabs[j - 1].nrows) {
        raise_index_error(ga.err);
        return 0.0f;
    }
    return to_f32(((const T*)ga.tabs[j - 1].data)[r * d + n]);
}

template <typename T, bool GATHER>
__global__ __launch_bounds__(256) void interact_bwd_scalar(int d, int F, int B, const T* __restrict__ dout,
                                                           int64_t dout_ld, const T* __restrict__ t, int64_t t_ld,
                                                           float* __restrict__ dx, int64_t dx_ld,
                                                           float* __restrict__ dt, int64_t dt_ld, GatherArgs ga,
                                                           const T* __restrict__ x, int64_t x_ld) {
    const int64_t total = (int64_t)B * F * d;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = e / ((int64_t)F * d);
        const int rem = (int)(e % ((int64_t)F * d));
        const int f = rem / d, n = rem % d;
        const T* ob = dout + b * dout_ld + d;
        float acc = 0.0f;
        for (int j = 0; j < F; ++j) {
            if (j == f) continue;
            const int hi = j > f ? j : f, lo = j > f ? f : j;
            acc = fmaf(t_elem<T, GATHER>(t, t_ld, b, j, n, d, ga, x, x_ld), to_f32(ob[hi * (hi - 1) / 2 + lo]), acc);
        }
        dt[b * dt_ld + (int64_t)f * d + n] = acc;
        if (f == 0) dx[b * dx_ld + n] = to_f32(dout[b * dout_ld + n]) + acc;
    }
}

// ------------------------------------------------------------------------ launchers
// Every launcher is interact_align -> plan_interact (interact_plan.hpp; DESIGN.md section 22 has the table) -> launch:
// the plan picks the kernel and its template arguments, with_elem / with_int turn them into types, and the grid and
// the dynamic LDS are sized here, beside the device types they come from.
static_assert(256 * kBwdIndexEPL == kBwdIndexMaxN, "interact_bwd_index_kernel's indexer and the plan's bound");

static unsigned grid_for(int64_t items, int per_block, int cus) {
    int64_t g = (items + per_block - 1) / per_block;
    const int64_t cap = (int64_t)cus * 16;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

// Run-time value -> compile-time: f(T{}) with the plan's element type; f(std::integral_constant<int, V>) with the V
// of Vs that n equals (false: none)
template <typename F> static void with_elem(bool f32, F&& f) { f32 ? f(float{}) : f(uint16_t{}); }
template <int... Vs, typename F> static bool with_int(int n, F&& f) {
    return ((n == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// The plan of a site (F = T_ + 1 features; the sites without tables pass tabs16 = true); htabs: the tables' host
// descriptors where the site may take their pointers by value
static InteractPlan plan_site(InteractSite site, bool tabs16, int T_, int dtype, int d, int B, int L, const void* x,
                              int64_t x_ld, const void* t = nullptr, int64_t t_ld = 0, const float* dx = nullptr,
                              int64_t dx_ld = 0, const float* dt = nullptr, int64_t dt_ld = 0,
                              const TableDesc* htabs = nullptr, int rule = kRuleDescent) {
    int64_t rows = htabs ? 0 : -1;
    for (int k = 0; htabs && k < T_; ++k) rows = htabs[k].nrows > rows ? htabs[k].nrows : rows;
    return plan_interact(site, InteractShape{dtype, d, T_ + 1, B, L, t != nullptr},
                         interact_align(dtype, d, x, x_ld, t, t_ld, dx, dx_ld, dt, dt_ld, tabs16, T_, rows), knobs(), rule);
}

// The tracing build holds the d = 128 forward at the shipped two workgroups per CU with unused
// dynamic LDS (16 KB static + 40 KB: two fit in 160 KB): the stamps change the kernel's register
// count, and a third workgroup would change the timeline they are there to show.
#ifdef DLRM_WTRACE
constexpr size_t kFwdTraceLds = 40 * 1024;
#else
constexpr size_t kFwdTraceLds = 0;
#endif

// interact_fwd_kernel (one wave per sample, 4 samples per workgroup) as the plan has it
template <bool FUSED>
static void launch_fwd(const InteractPlan& p, hipStream_t s, int cus, int d, int F, int B, const void* x, int64_t x_ld,
                       void* ys, int64_t ys_ld, void* out, int64_t out_ld, int padding, const GatherArgs& ga,
                       const TabPtrs& tp) {
    with_elem(p.f32, [&](auto e) {
        typedef decltype(e) T;
        const auto go = [&](auto kernel, size_t lds) {
            hipLaunchKernelGGL(kernel, dim3(grid_for(B, 4, cus)), dim3(256), lds, s, d, F, B, (const T*)x, x_ld, (T*)ys,
                               ys_ld, (T*)out, out_ld, padding, ga, tp);
        };
        with_int<1, 2, 3, 4, 5, 6>(p.NB, [&](auto nb) {
            constexpr int NB = decltype(nb)::value;
            if (FUSED && p.pooled) go(interact_fwd_kernel<T, NB, FUSED, true>, 0);
            else if (p.DC == 128) go(interact_fwd_kernel<T, NB, FUSED, false, 128>, kFwdTraceLds);
            else go(interact_fwd_kernel<T, NB, FUSED, false>, 0);
        });
    });
}

int launch_interact_fwd(dlrm_ctx* ctx, int dtype, int d, int F, int B, const void* x, int64_t x_ld, void* ys,
                        int64_t ys_ld, void* out, int64_t out_ld, int padding) {
    const InteractPlan p = plan_site(InteractSite::Fwd, true, F - 1, dtype, d, B, 1, x, x_ld, ys, ys_ld);
    if (p.kernel == InteractKernel::None) return p.rc;
    hipStream_t s = ctx_stream(ctx);
    const int cus = ctx_num_cus(ctx);
    if (p.kernel == InteractKernel::Fwd)
        launch_fwd<false>(p, s, cus, d, F, B, x, x_ld, ys, ys_ld, out, out_ld, padding, GatherArgs{}, TabPtrs{});
    else
        with_elem(p.f32, [&](auto e) {
            typedef decltype(e) T;
            const unsigned g = grid_for((int64_t)B * (d + F * (F - 1) / 2 + padding), 256, cus);
            hipLaunchKernelGGL(interact_fwd_scalar<T>, dim3(g), dim3(256), 0, s, d, F, B, (const T*)x, x_ld, (T*)ys, ys_ld,
                               (T*)out, out_ld, padding);
        });
    return ctx_hip(ctx, hipGetLastError(), "interact_fwd launch");
}

// maplookup(PreallocationStrategy(d)) + DotInteraction in one launch.  Returns
// DLRM_E_UNSUPPORTED when the shape/alignment has no fused kernel (the caller then runs
// the two operators separately).
int launch_lookup_interact_fwd(dlrm_ctx* ctx, const TableDesc* tabs, bool tabs_aligned16, int T_, int dtype,
                               const void* idx, int itype, int64_t tstride, int base, int L, int d, int B,
                               const void* x, int64_t x_ld, void* ys, int64_t ys_ld, void* out, int64_t out_ld,
                               int padding, const TableDesc* htabs) {
    const InteractPlan p = plan_site(InteractSite::LookupFwd, tabs_aligned16, T_, dtype, d, B, L, x, x_ld, ys, ys_ld,
                                     nullptr, 0, nullptr, 0, htabs);
    if (p.kernel == InteractKernel::None) return p.rc;
    GatherArgs ga{tabs, idx, itype, tstride, base, L, ctx_error_word(ctx)};
    TabPtrs tp{};
    if (p.tab_ptrs) fill_tab_ptrs(tp, htabs, T_);
    launch_fwd<true>(p, ctx_stream(ctx), ctx_num_cus(ctx), d, T_ + 1, B, x, x_ld, ys, ys_ld, out, out_ld, padding, ga, tp);
    return ctx_hip(ctx, hipGetLastError(), "lookup_interact_fwd launch");
}

// What the backward kernels share (t: a materialized ys, else x and ga's table rows)
struct BwdArgs {
    int d, F, B;
    const void* dout;
    int64_t dout_ld;
    const void* t;
    int64_t t_ld;
    float *dx, *dt;
    int64_t dx_ld, dt_ld;
    GatherArgs ga;
    const void* x;
    int64_t x_ld;
};

// interact_bwd_split_kernel: SPB samples per workgroup, WPS waves per sample, no dynamic LDS
template <typename T, int NB, int DC, int SPB, int WPS, bool MAPPED, int CPL, bool YS, typename SU>
static void launch_split(hipStream_t s, const BwdArgs& a, const SU& su) {
    hipLaunchKernelGGL((interact_bwd_split_kernel<T, NB, DC, SPB, WPS, MAPPED, CPL, YS, SU>),
                       dim3((unsigned)((a.B + SPB - 1) / SPB)), dim3(64 * WPS * SPB), 0, s, a.d, a.F, a.B, (const T*)a.dout,
                       a.dout_ld, a.dx, a.dx_ld, a.dt, a.dt_ld, a.ga, (const T*)(YS ? a.t : a.x), YS ? a.t_ld : a.x_ld, su);
}

// dT = S T per sample by the kernels without an update: T from a.t or, gather, from x + the table rows; mapped (the
// blocked backward): dt is the send layout
static int launch_bwd(dlrm_ctx* ctx, const InteractPlan& p, const BwdArgs& a, const char* what) {
    typedef InteractKernel K;
    hipStream_t s = ctx_stream(ctx);
    const int cus = ctx_num_cus(ctx);
    const StepUpdate su{nullptr, 0, 0.0f, ctx_error_word(ctx)};
    with_elem(p.f32, [&](auto e) {
        typedef decltype(e) T;
        const auto go = [&](auto kernel, unsigned g, int threads, size_t lds) {
            hipLaunchKernelGGL(kernel, dim3(g), dim3(threads), lds, s, a.d, a.F, a.B, (const T*)a.dout, a.dout_ld,
                               (const T*)a.t, a.t_ld, a.dx, a.dx_ld, a.dt, a.dt_ld, a.ga, (const T*)a.x, a.x_ld);
        };
        with_int<0, 1>(p.gather, [&](auto gather) {
            constexpr bool GATHER = decltype(gather)::value != 0;
            if (p.kernel == K::BwdScalar)
                go(interact_bwd_scalar<T, GATHER>, grid_for((int64_t)a.B * a.F * a.d, 256, cus), 256, 0);
            else if (p.kernel == K::Bwd)
                with_int<1, 2, 3, 4, 5, 6, 7>(p.NB, [&](auto nb) {
                    typedef BwdGeom<decltype(nb)::value> G;
                    go(interact_bwd_kernel<T, decltype(nb)::value, GATHER>, grid_for(a.B, G::WPB, cus), 64 * G::WPB,
                       sizeof(float) * G::LDS_FLOATS * G::WPB + (GATHER ? (sizeof(TableDesc) + 16) * (a.F - 1) : 0));
                });
        });
        if (p.kernel == K::BwdSplit && p.ys)
            with_int<3, 4, 5, 6>(p.NB, [&](auto nb) {
                with_int<1, 2, 4>(p.WPS, [&](auto w) {
                    launch_split<T, decltype(nb)::value, 0, 1, decltype(w)::value, false, 4, true>(s, a, su);
                });
            });
        else if (p.kernel == K::BwdSplit)
            with_int<1, 2>(p.NB, [&](auto nb) {
                if (p.DC == 128) launch_split<T, decltype(nb)::value, 128, 4, 2, true, 4, false>(s, a, su);
                else launch_split<T, decltype(nb)::value, 0, 2, 1, true, 4, false>(s, a, su);
            });
    });
    return ctx_hip(ctx, hipGetLastError(), what);
}

int launch_interact_bwd(dlrm_ctx* ctx, int dtype, int d, int F, int B, const void* dout, int64_t dout_ld,
                        const void* t, int64_t t_ld, float* dx, int64_t dx_ld, float* dt, int64_t dt_ld) {
    const InteractPlan p = plan_site(InteractSite::Bwd, true, F - 1, dtype, d, B, 1, nullptr, 0, t, t_ld, dx, dx_ld, dt, dt_ld);
    if (p.kernel == InteractKernel::None) return p.rc;
    return launch_bwd(ctx, p, BwdArgs{d, F, B, dout, dout_ld, t, t_ld, dx, dt, dx_ld, dt_ld, GatherArgs{}, nullptr, 0},
                      p.ys ? "interact_bwd(ys, split) launch" : "interact_bwd launch");
}

int launch_interact_bwd_gather(dlrm_ctx* ctx, const TableDesc* tabs, bool tabs_aligned16, int T_, int dtype,
                               const void* idx, int itype, int64_t tstride, int base, int L, int d, int B,
                               const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, float* dx,
                               int64_t dx_ld, float* dt, int64_t dt_ld, const IndexerDev* ix) {
    const InteractPlan p = plan_site(ix ? InteractSite::BwdGatherIndexed : InteractSite::BwdGather, tabs_aligned16, T_, dtype,
                                     d, B, L, x, x_ld, nullptr, 0, dx, dx_ld, dt, dt_ld);
    const int F = T_ + 1;
    const GatherArgs ga{tabs, idx, itype, tstride, base, L, ctx_error_word(ctx)};
    if (p.kernel == InteractKernel::BwdIndex) {
        with_elem(p.f32, [&](auto e) {
            typedef decltype(e) T;
            with_int<1, 2>(p.NB, [&](auto nb) {
                typedef BwdGeom<decltype(nb)::value> G;
                size_t lds = sizeof(FastLds<256, kBwdIndexEPL>);
                const size_t blds = sizeof(float) * G::LDS_FLOATS * G::WPB + sizeof(TableDesc) * T_;
                if (blds > lds) lds = blds;
                hipLaunchKernelGGL((interact_bwd_index_kernel<T, decltype(nb)::value>),
                                   dim3(grid_for(B, G::WPB, ctx_num_cus(ctx)) + T_), dim3(256), lds, ctx_stream(ctx), d, F, B,
                                   (const T*)dout, dout_ld, dx, dx_ld, dt, dt_ld, ga, (const T*)x, x_ld, *ix);
            });
        });
        return ctx_hip(ctx, hipGetLastError(), "interact_bwd(+indexer) launch");
    }
    if (p.build_first) {
        const int rc = launch_indexer_build(ctx, *ix, tabs, T_, idx, itype, tstride, base, B, L,
                                            standalone_form((int64_t)B * L, ix->hsize, false), false,
                                            ctx_error_word(ctx));
        if (rc) return rc;
    }
    if (p.kernel == InteractKernel::None) return p.rc;
    return launch_bwd(ctx, p, BwdArgs{d, F, B, dout, dout_ld, nullptr, 0, dx, dt, dx_ld, dt_ld, ga, x, x_ld},
                      "interact_bwd launch");
}

// dlrm_interact_bwd_gather with table t's dt rows written to dst + dbase[t] + b * dld[t] (the
// sharded exchange's send layout) by the backward's own stores: no dt buffer, no repack launch.
// Vector kernel shapes only (DLRM_E_UNSUPPORTED otherwise).
int launch_interact_bwd_blocked(dlrm_ctx* ctx, const TableDesc* tabs, bool tabs_aligned16, int T_, int dtype,
                                const void* idx, int itype, int64_t tstride, int base, int L, int d, int B,
                                const void* x, int64_t x_ld, const void* dout, int64_t dout_ld, float* dx,
                                int64_t dx_ld, float* dst, const int64_t* dbase, const int64_t* dld) {
    const InteractPlan p = plan_site(InteractSite::BwdBlocked, tabs_aligned16, T_, dtype, d, B, L, x, x_ld, nullptr, 0, dx,
                                     dx_ld, dst, 0);
    if (p.rc) return ctx_fail(ctx, p.rc, "interact_bwd_blocked: 16-B aligned rows and F <= 112 needed");
    if (p.kernel == InteractKernel::None) return DLRM_OK;
    const GatherArgs ga{tabs, idx, itype, tstride, base, L, ctx_error_word(ctx), dbase, dld};
    return launch_bwd(ctx, p, BwdArgs{d, T_ + 1, B, dout, dout_ld, nullptr, 0, dx, dst, dx_ld, 0, ga, x, x_ld},
                      p.kernel == InteractKernel::BwdSplit ? "interact_bwd_blocked(split) launch"
                                                           : "interact_bwd_blocked launch");
}

// Whether a shape has a kernel, asked before a build is planned (build_plan.hpp BuildCaps): the launchers' own plans.
// The step backward's take one sample: no batch size changes whether a kernel exists.
bool lookup_fwd_supported(bool tabs_aligned16, int T_, int dtype, int d, int B, const void* x, int64_t x_ld,
                          const TableDesc* htabs) {
    return plan_site(InteractSite::LookupFwd, tabs_aligned16, T_, dtype, d, B, 1, x, x_ld, nullptr, 0, nullptr, 0, nullptr, 0,
                     htabs).rc == DLRM_OK;
}
bool step_fwd_supported(bool tabs_aligned16, int T_, int dtype, int d, int B, const void* x, int64_t x_ld,
                        const TableDesc* htabs) {
    return plan_site(InteractSite::StepFwd, tabs_aligned16, T_, dtype, d, B, 1, x, x_ld, nullptr, 0, nullptr, 0, nullptr, 0,
                     htabs).rc == DLRM_OK;
}
bool step_bwd_supported(int kind, bool tabs_aligned16, int T_, int dtype, int d, const void* x, int64_t x_ld) {
    return plan_site(InteractSite::StepBwd, tabs_aligned16, T_, dtype, d, 1, 1, x, x_ld, nullptr, 0, nullptr, 0, nullptr, 0,
                     nullptr, kind).kernel != InteractKernel::None;
}
bool step_split_supported(bool tabs_aligned16, int T_, int dtype, int d, const void* x, int64_t x_ld) {
    return step_bwd_supported(kRuleDescent, tabs_aligned16, T_, dtype, d, x, x_ld);
}

// Training-step forward (split indexer in the same grid).  DLRM_E_UNSUPPORTED when the shape
// has no such kernel (the caller then runs the fused forward and the indexer separately).
int launch_step_fwd(dlrm_ctx* ctx, const TableDesc* tabs, bool tabs_aligned16, int T_, int dtype, const void* idx,
                    int itype, int64_t tstride, int base, int d, int B, const void* x, int64_t x_ld, void* out,
                    int64_t out_ld, int padding, const IndexerDev& ix, const TableDesc* htabs) {
    const InteractPlan p = plan_site(InteractSite::StepFwd, tabs_aligned16, T_, dtype, d, B, 1, x, x_ld, nullptr, 0, nullptr,
                                     0, nullptr, 0, htabs);
    if (p.kernel == InteractKernel::None) return p.rc;
    const GatherArgs ga{tabs, idx, itype, tstride, base, 1, ctx_error_word(ctx)};
    TabPtrs tp{};
    fill_tab_ptrs(tp, htabs, T_);
    const bool wave = ix.vshift >= 2;
    size_t lds = wave ? sizeof(WaveBuildLds) : sizeof(StepLds);
    if (lds < sizeof(float) * 4 * kStage) lds = sizeof(float) * 4 * kStage;
    const unsigned g = grid_for(B, 4, ctx_num_cus(ctx)) + (wave ? (T_ << ix.vshift) / kWaveParts : (T_ << ix.vshift));
    with_elem(p.f32, [&](auto e) {
        typedef decltype(e) T;
        const auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(g), dim3(256), lds, ctx_stream(ctx), d, T_ + 1, B, (const T*)x, x_ld, (T*)out,
                               out_ld, padding, ga, ix, tp);
        };
        with_int<1, 2>(p.NB, [&](auto nb) {
            if (p.DC == 128) go(interact_fwd_index_kernel<T, decltype(nb)::value, 128>);
            else go(interact_fwd_index_kernel<T, decltype(nb)::value>);
        });
    });
    return ctx_hip(ctx, hipGetLastError(), "step_fwd launch");
}

// the kRule* of a StepUpdate type
template <typename SU>
constexpr int rule_of() {
    if (SU::kStochastic && SU::kAdagrad != 0) return SU::kAdagrad == 2 ? kRuleStochasticRowwise : kRuleStochasticAdagrad;
    return SU::kSplit ? kRuleSplit
                      : (SU::kStochastic ? kRuleStochastic
                                         : (SU::kAdagrad == 2 ? kRuleRowwise : (SU::kAdagrad == 1 ? kRuleAdagrad : kRuleDescent)));
}

// Training-step backward after launch_step_fwd under the rule SU: once-hit rows updated in place, dt rows of the
// others written for the apply.  (A form step_bwd_form leaves out is not instantiated.)
template <typename T, typename SU>
static int launch_step_bwd_rule(dlrm_ctx* ctx, const InteractPlan& p, const BwdArgs& a, const SU& su) {
    [[maybe_unused]] constexpr bool f32 = sizeof(T) == 4, descent = rule_of<SU>() == kRuleDescent;
    hipStream_t s = ctx_stream(ctx);
    bool done = false;
    if (p.kernel == InteractKernel::BwdSplit) {
        with_int<1, 2>(p.NB, [&](auto nb) {
            with_int<1, 2>(p.WPS, [&](auto w) {
                with_int<4, 8>(p.CPL, [&](auto c) {
                    with_int<8, 4, 2>(p.SPB, [&](auto spb) {
                        constexpr int NB = decltype(nb)::value, WPS = decltype(w)::value, CPL = decltype(c)::value;
                        constexpr int SPB = decltype(spb)::value, DC = WPS == 2 || CPL == 8 ? 128 : 0;
                        if constexpr (step_bwd_form(rule_of<SU>(), f32, NB, WPS, CPL, SPB)) {
                            launch_split<T, NB, DC, SPB, WPS, false, CPL, false, SU>(s, a, su);
                            done = true;
                        }
                    });
                });
            });
        });
    } else if constexpr (SU::kAdagrad == 0 && !SU::kStochastic) {  // interact_bwd_update_kernel: Descent, the split rule
        if (p.kernel == InteractKernel::BwdUpdate) with_int<1, 2>(p.NB, [&](auto nb) {
            with_int<1, 2>(p.SBU, [&](auto sbu) {
                with_int<0, 128>(p.DC, [&](auto dc) {
                    constexpr int NB = decltype(nb)::value, SBU = decltype(sbu)::value, DC = decltype(dc)::value;
                    if constexpr (descent ? (SBU == 1 || DC == 128) : (SBU == 1 && DC == 0)) {
                        typedef BwdGeom<NB> G;
                        const size_t lds = sizeof(float) * G::template lds_floats<true>() * G::WPB +
                                           (sizeof(TableDesc) + (SU::kSplit ? sizeof(void*) : 0)) * (a.F - 1);
                        hipLaunchKernelGGL((interact_bwd_update_kernel<T, NB, SBU, DC, SU>),
                                           dim3(grid_for(a.B, G::WPB, ctx_num_cus(ctx))), dim3(64 * G::WPB), lds, s, a.d, a.F,
                                           a.B, (const T*)a.dout, a.dout_ld, a.dx, a.dx_ld, a.dt, a.dt_ld, a.ga,
                                           (const T*)a.x, a.x_ld, su);
                        done = true;
                    }
                });
            });
        });
    }
    if (!done) return ctx_fail(ctx, DLRM_E_UNSUPPORTED, "%s: no kernel for this shape", SU::kName);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return DLRM_OK;
    const char* const form = p.kernel == InteractKernel::BwdUpdate ? ""
                             : p.CPL == 8 ? (SU::kAdagrad ? "(8 columns per lane)" : "(split)")
                                          : (p.WPS == 2 ? "(split)" : "(one wave per sample)");
    return ctx_hip(ctx, e, (std::string(SU::kName) + form + " launch").c_str());
}

// The one launcher of the public step backward: the arguments every rule shares, then the rule's StepUpdate type (and,
// where the rule takes fp32 tables, the element type).  The caller checked the shape (has_split_bwd: 16-B aligned
// table rows among it), the 16-B alignment of dx / dt and of the rule's second stream, and bf16 tables for the rules
// that need them.
int launch_step_bwd(dlrm_ctx* ctx, const TableDesc* tabs, int T_, int dtype, const void* idx, int itype,
                    int64_t tstride, int base, int d, int B, const void* x, int64_t x_ld, const void* dout,
                    int64_t dout_ld, float* dx, int64_t dx_ld, float* dt, int64_t dt_ld, const IndexerDev& ix,
                    const BoundRule& r) {
    const InteractPlan p = plan_site(InteractSite::StepBwd, true, T_, dtype, d, B, 1, x, x_ld, nullptr, 0, nullptr, 0, nullptr,
                                     0, nullptr, r.kind);
    if (p.kernel == InteractKernel::None && p.rc == DLRM_OK) return DLRM_OK;  // (a refusal: the rule's message below)
    const GatherArgs ga{tabs, idx, itype, tstride, base, 1, ctx_error_word(ctx)};
    const BwdArgs a{d, T_ + 1, B, dout, dout_ld, nullptr, 0, dx, dt, dx_ld, dt_ld, ga, x, x_ld};
    const StepUpdate su{ix.single, ix.cap, r.lr, ctx_error_word(ctx)};
    float* const* const state = (float* const*)r.state;
    const uint32_t k0 = (uint32_t)r.seed, k1 = (uint32_t)(r.seed >> 32);
    const auto run = [&](auto e, const auto& rule) { return launch_step_bwd_rule<decltype(e)>(ctx, p, a, rule); };
    switch (r.kind) {
        case kRuleSplit: return run(uint16_t{}, SplitStepUpdate{su, (uint16_t* const*)r.state});
        case kRuleStochastic:
            return run(uint16_t{}, StochasticStepUpdate{su, (uint32_t)r.seed, (uint32_t)(r.seed >> 32), r.step});
        case kRuleAdagrad:
            return p.f32 ? run(float{}, AdagradStepUpdate<false>{su, state, r.eps})
                         : run(uint16_t{}, AdagradStepUpdate<false>{su, state, r.eps});
        case kRuleRowwise:
            return p.f32 ? run(float{}, AdagradStepUpdate<true>{su, state, r.eps})
                         : run(uint16_t{}, AdagradStepUpdate<true>{su, state, r.eps});
        default: return p.f32 ? run(float{}, su) : run(uint16_t{}, su);
        // (the seeded Adagrad rules last: their kernels are emitted behind every other of the unit)
        case kRuleStochasticAdagrad:
            return run(uint16_t{}, StochasticAdagradStepUpdate<false>{{su, state, r.eps}, k0, k1, r.step});
        case kRuleStochasticRowwise:
            return run(uint16_t{}, StochasticAdagradStepUpdate<true>{{su, state, r.eps}, k0, k1, r.step});
    }
}

}  // namespace dlrm
