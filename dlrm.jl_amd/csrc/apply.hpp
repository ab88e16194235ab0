// apply.hpp — the work items of EmbeddingTables.update!(Descent(lr), ...) (sgd_apply_kernel).
//
// Reference: src/train/train.jl:283-290 (update! over the SparseIndexer's grouping), pinned by
// src/validation.jl:125-146.  Work items of the indexer (indexer.hpp):
//   * a chunk: a segment (one table row) of <= kChunk positions, run by one lane group: the grad
//     rows are summed in ascending position order from 0, then w = fmaf(-lr, sum, w);
//   * a slice: <= kHotSlice consecutive positions of a longer (hot) segment, run by a whole
//     256-thread workgroup: each lane group sums its consecutive share of the slice in position
//     order, the groups of a wave are combined by a fixed xor butterfly, the waves in wave order.
//     A one-slice segment then updates its row; otherwise the slice stores its partial row
//     (write-through) and adds to the segment's arrival counter, and the last arriving slice adds
//     the partials in slice order from 0 and updates the row.
// Every touched row is written exactly once with a summation order fixed by its positions alone,
// so the result is bitwise reproducible.
//
// Latency is what bounds these items (a few dependent memory round trips each), so a chunk's
// first kChunkInline positions come with its descriptor, the rest with one load per lane, and up
// to 16 grad rows are in flight per lane group.
#pragma once
#include "indexer.hpp"

namespace dlrm {

constexpr int kApplyThreads = 256;
#ifndef DLRM_SLICE_IF
#define DLRM_SLICE_IF 16
#endif
constexpr int kSliceIF = DLRM_SLICE_IF;  // hot slice: grad rows in flight per lane (16-B rows)
constexpr int kApplyWaves = kApplyThreads / 64;

// Lane-group geometry: D elements = VPR vectors of 16 B of the GRAD dtype; a group of LPR lanes
// owns one row, a wave holds RPW groups.
template <typename GT, int VPR>
struct ApplyGeom {
    typedef Vec<GT> GV;
    static constexpr int NE = GV::N;
    static constexpr int D = VPR * NE;
    static constexpr int LPR = VPR <= 64 ? VPR : 64;
    static constexpr int VPL = VPR <= 64 ? 1 : VPR / 64;
    static constexpr int RPW = 64 / LPR;
    static constexpr int NG = kApplyWaves * RPW;        // lane groups per workgroup
    static constexpr int SIF = NE == 8 ? kSliceIF / 2 : kSliceIF;  // hot slice rows in flight (bf16: 8 per 16 B)
    static constexpr int IF = VPL >= 4 ? 4 : (NE == 8 ? 8 : 16) / VPL;  // grad rows in flight per lane
    // once-hit positions per lane group (a grad and a table row in flight for each; a rule with
    // state in flight beside the table row takes fewer: its singles_ppg)
    static constexpr int SPPG = VPL * NE >= 16 ? 2 : (VPL * NE >= 8 ? 4 : 8);
};

// Cross-workgroup hand-off of slice partials (cdna_hip_programming.md Guideline 16, R1/R2):
// payload stored write-through (agent-scope atomic stores = sc1), the storing wave drains
// (vmcnt(0)) before ONE lane adds to the segment's arrival counter; the last arriver reads every
// partial with sc1 loads (no acquire needed) and resets the counter for the next launch.
typedef __attribute__((address_space(1))) unsigned long long gu64_t;
typedef __attribute__((address_space(1))) int gi32_t;

__device__ __forceinline__ void store_sc1(float* p, const f32x4& v) {
    const unsigned long long lo = ((unsigned long long)__float_as_uint(v[1]) << 32) | __float_as_uint(v[0]);
    const unsigned long long hi = ((unsigned long long)__float_as_uint(v[3]) << 32) | __float_as_uint(v[2]);
    __hip_atomic_store((gu64_t*)p, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((gu64_t*)(p + 2), hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ f32x4 load_sc1(const float* p) {
    const unsigned long long lo = __hip_atomic_load((gu64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long hi = __hip_atomic_load((gu64_t*)(p + 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return f32x4{__uint_as_float((uint32_t)lo), __uint_as_float((uint32_t)(lo >> 32)), __uint_as_float((uint32_t)hi),
                 __uint_as_float((uint32_t)(hi >> 32))};
}

// The grad row of position p, vector k of this lane (k = v + j*64).
template <typename GT>
__device__ __forceinline__ typename Vec<GT>::type grad_vec(const GT* gbase, int64_t grad_ld, const FastDiv& L, int p, int k) {
    return ldg<typename Vec<GT>::type>((const typename Vec<GT>::type*)(gbase + (int64_t)L(p) * grad_ld) + k);
}

template <typename GT>
__device__ __forceinline__ void add_vec(float* acc, const typename Vec<GT>::type& g) {
    float f[Vec<GT>::N];
    Vec<GT>::to_f32(g, f);
#pragma unroll
    for (int e = 0; e < Vec<GT>::N; ++e) acc[e] += f[e];
}

// ---- update rules: what a touched row's write does with its complete gradient sum G (fp32).
//   Descent         w = fmaf(-lr, G, w)
//   Adagrad         A += G^2 (element-wise, fp32 [nrows][D]);   w -= lr G / (sqrt(A) + eps)
//   RowwiseAdagrad  m += (1/D) sum_c G[c]^2 (fp32 [nrows]);      w -= lr G / (sqrt(m) + eps)
//   SplitDescent    W = bits(hi << 16 | lo);  W' = fmaf(-lr, G, W);  hi' = bits(W') >> 16, lo' = bits(W') & 0xffff
//                   (hi = the bf16 table's element, lo = a uint16 [nrows][D] state row: the table holds
//                   the truncated high half of an fp32 master weight, the step is Descent's on fp32)
//   StochasticDescent  W' = fmaf(-lr, G, w);  w = sr_bf16(W', R): Descent on bf16 tables whose store rounds W' up
//                   or down with probability proportional to its distance to each bf16 neighbour (no state; R =
//                   16 Philox bits of (seed, step, table, row, column), below)
//   StochasticAdagrad, StochasticRowwiseAdagrad  the Adagrad rules on bf16 tables with that store: the parent's G, state
//                   and W', w = sr_bf16(W', R) (below StochasticDescent)
// A rule holds its parameters, its state's row address (state_row), its once-hit positions per lane group
// (singles_ppg), the any-D kernels' write of one column (scalar_write) and the MODEs and table element types
// it is instantiated for (kCarriesBuild, kBuildWithApply, kF32Tables), and whether its store of the weights is the
// stochastic one (kStochastic: rule_store then calls its store<NE>, and the kernels its load_step).  The vector items below still branch on kState (0 none,
// 1 a state row per table row, 2 a state word, 3 a row of low halves, 4 none: StochasticDescent): written once over a per-rule row type
// they no longer compiled to the same code.  The state is loaded where the table row
// is (beside the grad rows: these items are bound by dependent round trips) and written once, with the row.

// N (4 or 8) consecutive 16-bit halves of a split row, kept as raw bits in one 8-B or 16-B vector (half
// the registers of their fp32 values while they wait beside the grad rows).
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
template <int N> struct Halves;
template <> struct Halves<4> { typedef u16x4 type; };
template <> struct Halves<8> { typedef u16x8 type; };
template <int N>
__device__ __forceinline__ typename Halves<N>::type load_halves(const uint16_t* p) {
    return ldg<typename Halves<N>::type>(p);
}
// the split step on N elements: the fp32 master weight from its halves, Descent's fma, the halves of
// the result by truncation.  A NaN result also sets the high half's quiet bit (as f32_to_bf16 does), so
// the bf16 table alone still reads NaN when the payload sits in the low half.
__device__ __forceinline__ void split_step1(float lr, float g, uint16_t& hi, uint16_t& lo) {
    const float w = __builtin_fmaf(-lr, g, __uint_as_float(((uint32_t)hi << 16) | (uint32_t)lo));
    const uint32_t u = __float_as_uint(w);
    hi = (uint16_t)((u >> 16) | (w != w ? 0x40u : 0u));
    lo = (uint16_t)(u & 0xffffu);
}
template <int N>
__device__ __forceinline__ void split_step(float lr, const float* g, typename Halves<N>::type& hi,
                                           typename Halves<N>::type& lo) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
        uint16_t h = hi[e], l = lo[e];
        split_step1(lr, g[e], h, l);
        hi[e] = h;
        lo[e] = l;
    }
}
// ... and its write: both halves of the N elements at `hrow` / `lrow`, one vector store each
template <int N>
__device__ __forceinline__ void split_write(float lr, const float* g, typename Halves<N>::type& hi,
                                            typename Halves<N>::type& lo, uint16_t* hrow, uint16_t* lrow) {
    split_step<N>(lr, g, hi, lo);
    stg<typename Halves<N>::type>(hrow, hi);
    stg<typename Halves<N>::type>(lrow, lo);
}

// The element-wise rule's sqrt and reciprocal: the hardware's (v_sqrt_f32, v_rcp_f32: 1 ulp each)
// instead of the correctly rounded expansions (~25 instructions and 6 live registers per element,
// times up to 32 elements in flight per lane in a singles item).  Their operands are normal
// numbers (A >= its initial eps > 0); the step stays within 4 ulp of the exact quotient.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
#else  // host pass of the device code: never executed
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ float fast_rcp(float x) { return 1.0f / x; }
#endif

// N elements of a row: a (the Adagrad accumulators) and w updated from the sums g
template <int N>
__device__ __forceinline__ void adagrad_step(float lr, float eps, const float* g, float* a, float* w) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
        a[e] = __builtin_fmaf(g[e], g[e], a[e]);
        w[e] = __builtin_fmaf(-lr, g[e] * fast_rcp(fast_sqrt(a[e]) + eps), w[e]);
    }
}
template <int N>
__device__ __forceinline__ float sum_squares(const float* g, float ss) {
#pragma unroll
    for (int e = 0; e < N; ++e) ss = __builtin_fmaf(g[e], g[e], ss);
    return ss;
}
// the row-wise accumulator after a row whose squares sum to ss, and the row's step size
__device__ __forceinline__ float rowwise_m(float m, float ss, int D) { return m + ss / (float)D; }
__device__ __forceinline__ float rowwise_scale(float lr, float eps, float m) { return lr / (__builtin_sqrtf(m) + eps); }

// A rule with a state row or word in flight beside each table row takes SPPG / DIV once-hit positions per
// lane group.  The MODE 1 kernels sit at the 168-register limit of three workgroups per CU; at SPPG the
// Adagrad instantiations spill up to 1300 registers to scratch, with these counts none does.
constexpr int fewer_singles(int sppg, int div) { return sppg >= div ? sppg / div : 1; }

struct Descent {
    float lr;
    typedef float State;
    static constexpr int kState = 0;  // (the items' per-rule branches: 0 none, 1 a state row, 2 a state word, 3 low halves)
    static constexpr bool kStochastic = false;  // (rule_store: the weights' store rounds to nearest)
    static constexpr bool kCarriesBuild = true;  // MODE >= 2: the next batch's build rides on its launches
    static constexpr bool kBuildWithApply = true;  // ... instantiated where its MODE 0 / 1 launches are
    static constexpr bool kF32Tables = true;
    __device__ __forceinline__ float* base(int) const { return nullptr; }
    template <int D> __device__ static __forceinline__ float* state_row(float*, uint32_t) { return nullptr; }
    template <typename G> static constexpr int singles_ppg() { return G::SPPG; }
    static constexpr int scalar_threads(int D) { return D; }  // any-D kernels: threads per row
    template <typename TT, typename F>
    __device__ __forceinline__ void scalar_write(TT* __restrict__ row, float*, int64_t, int, int c, int, F&& colsum) const {
        row[c] = from_f32<TT>(__builtin_fmaf(-lr, colsum(c), to_f32(row[c])));
    }
};

struct Adagrad {
    float lr, eps;
    float* const* state;  // [T] device pointers, fp32 [nrows][D]
    typedef float State;
    static constexpr int kState = 1;
    static constexpr bool kStochastic = false;
    // MODE >= 2 over the training step's fp32 dt, in a unit of its own (adagrad_step.hip:
    // launch_adagrad_step_apply), so adagrad.hip stays the MODE 0 / 1 unit it was
    static constexpr bool kCarriesBuild = true;
    static constexpr bool kBuildWithApply = false;
    static constexpr bool kF32Tables = true;
    __device__ __forceinline__ float* base(int t) const { return ldg<float*>(state + t); }
    template <int D> __device__ static __forceinline__ float* state_row(float* st, uint32_t r) { return st + (int64_t)r * D; }
    // (a state row per table row: a quarter of SPPG for fp32 gradient rows, else half)
    template <typename G> static constexpr int singles_ppg() { return fewer_singles(G::SPPG, G::NE == 4 ? 4 : 2); }
    static constexpr int scalar_threads(int D) { return D; }
    template <typename TT, typename F>
    __device__ __forceinline__ void scalar_write(TT* __restrict__ row, float* __restrict__ st, int64_t r, int D, int c, int,
                                                 F&& colsum) const {
        const float g = colsum(c);
        float a = st[r * D + c], w = to_f32(row[c]);
        adagrad_step<1>(lr, eps, &g, &a, &w);
        st[r * D + c] = a;
        row[c] = from_f32<TT>(w);
    }
};

// The row-wise sum of squares has a fixed order per site: a lane's elements in element order, then an
// xor butterfly over the lanes holding the row (every level one commutative add, so every lane ends
// with the same bits), then (slices of D > 256) the waves in wave order.
struct RowwiseAdagrad {
    float lr, eps;
    float* const* state;  // [T] device pointers, fp32 [nrows]
    typedef float State;
    static constexpr int kState = 2;
    static constexpr bool kStochastic = false;
    // (MODE >= 2: adagrad_rowwise_step.hip, launch_rowwise_adagrad_step_apply)
    static constexpr bool kCarriesBuild = true;
    static constexpr bool kBuildWithApply = false;
    static constexpr bool kF32Tables = true;
    __device__ __forceinline__ float* base(int t) const { return ldg<float*>(state + t); }
    template <int D> __device__ static __forceinline__ float* state_row(float* st, uint32_t r) { return st + r; }
    // (a state word per table row: a quarter of SPPG for fp32 gradient rows of one vector per lane, else half)
    template <typename G> static constexpr int singles_ppg() { return fewer_singles(G::SPPG, G::NE == 4 && G::VPL == 1 ? 4 : 2); }
    static constexpr int scalar_threads(int) { return 1; }  // (two passes over the row's sums)
    // (c = 0: the thread has the whole row; the squares in column order, then the step)
    template <typename TT, typename F>
    __device__ __forceinline__ void scalar_write(TT* __restrict__ row, float* __restrict__ st, int64_t r, int D, int, int,
                                                 F&& colsum) const {
        float ss = 0.0f;
        for (int k = 0; k < D; ++k) {
            const float g = colsum(k);
            ss = __builtin_fmaf(g, g, ss);
        }
        const float m = rowwise_m(st[r], ss, D);
        const float s = rowwise_scale(lr, eps, m);
        st[r] = m;
        for (int k = 0; k < D; ++k) row[k] = from_f32<TT>(__builtin_fmaf(-s, colsum(k), to_f32(row[k])));
    }
};

struct SplitDescent {
    float lr;
    uint16_t* const* lo;  // [T] device pointers, uint16 [nrows][D]: the low halves
    typedef uint16_t State;
    static constexpr int kState = 3;
    static constexpr bool kStochastic = false;
    // MODE >= 2 over bf16 tables and the training step's fp32 dt, in a unit of their own (split_step.hip:
    // launch_split_step_apply), so split_sgd.hip stays the MODE 0 / 1 unit it was
    static constexpr bool kCarriesBuild = true;
    static constexpr bool kBuildWithApply = false;
    static constexpr bool kF32Tables = false;  // split rows live in bf16 tables
    __device__ __forceinline__ uint16_t* base(int t) const { return ldg<uint16_t*>(lo + t); }
    template <int D> __device__ static __forceinline__ uint16_t* state_row(uint16_t* st, uint32_t r) { return st + (int64_t)r * D; }
    // The split rule's halves wait as bits, a row's two halves in the registers of Descent's fp32 row, so
    // it keeps SPPG -- but for fp32 gradient rows of 16 vectors (D = 64), whose MODE 1 kernel spilt 4
    // registers at SPPG = 8: half as many there.
    template <typename G> static constexpr int singles_ppg() { return G::NE == 4 && G::LPR == 16 ? G::SPPG / 2 : G::SPPG; }
    static constexpr int scalar_threads(int D) { return D; }
    template <typename TT, typename F>
    __device__ __forceinline__ void scalar_write(TT* __restrict__ row, uint16_t* __restrict__ st, int64_t r, int D, int c, int,
                                                 F&& colsum) const {
        static_assert(sizeof(TT) == 2, "split rows live in bf16 tables");
        const float g = colsum(c);
        uint16_t h = ldg<uint16_t>(row + c), l = ldg<uint16_t>(st + r * D + c);
        split_step1(lr, g, h, l);
        stg<uint16_t>(row + c, h);
        stg<uint16_t>(st + r * D + c, l);
    }
};

// ---- stochastic rounding (StochasticDescent).  sr_bf16(W', R), u = bits(W'): an Inf or a NaN goes through
// f32_to_bf16 (NaN keeps its quiet bit), anything else is (u + R) >> 16 with R uniform in [0, 65536): the
// magnitude rounds away from zero with probability (u & 0xffff) / 65536 exactly, a W' that is a bf16 value is
// kept, and a finite W' above the largest finite bf16 can reach Inf, its upper neighbour.
__device__ __forceinline__ uint16_t sr_bf16(float w, uint32_t R) {
    const uint32_t u = __float_as_uint(w);
    if ((u & 0x7f800000u) == 0x7f800000u) return f32_to_bf16(w);
    return (uint16_t)((u + R) >> 16);
}
// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key (k0, k1); c becomes the output block
__device__ __forceinline__ void philox4x32_10(uint32_t* c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c[0]), l0 = 0xD2511F53u * c[0];
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c[2]), l1 = 0xCD9E8D57u * c[2];
        c[0] = h1 ^ c[1] ^ k0;
        c[1] = l1;
        c[2] = h0 ^ c[3] ^ k1;
        c[3] = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// R of element (table t, row r, column c) at step s under the seed is a function of those alone -- not of the
// indexer's form, its chunk limit or parts, or the launch or lane that writes the row: key = (seed lo, seed hi),
// counter = (r, t << 16 | c >> 2, s lo, s hi), and column c takes the low 16 bits of output word c & 3.  One block
// serves four consecutive columns, generated at the write (after the loads: nothing is held across the gather).
// The step is one device word the optimizer handle owns: every launch of an update call reads it (load_step, once
// per workgroup into scalars) and a one-thread launch after the call's last adds one, in stream order.  The fused
// training step with the rule (dlrm_sr_step_bwd) is one value of the word: its backward (interact.hip: this struct's
// load_step and store at the once-hit write) and its apply read the same value, and the advance follows the apply.
// No per-row state, so the rule alternates freely with Descent on the same tables.
struct StochasticDescent {
    float lr;
    uint32_t k0, k1;       // the seed's halves
    const uint64_t* step;  // the handle's step word
    uint32_t s0, s1;       // its value, by load_step
    typedef float State;
    static constexpr int kState = 4;
    static constexpr bool kStochastic = true;  // (rule_store: its store<NE>; the kernels call its load_step)
    // MODE >= 2 over the training step's fp32 dt, in a unit of its own (sr_step.hip: launch_sr_step_apply), so
    // sr_sgd.hip stays the MODE 0 / 1 unit it was
    static constexpr bool kCarriesBuild = true;
    static constexpr bool kBuildWithApply = false;
    static constexpr bool kF32Tables = false;  // fp32 tables: nothing to round
    __device__ __forceinline__ float* base(int) const { return nullptr; }
    template <int D> __device__ static __forceinline__ float* state_row(float*, uint32_t) { return nullptr; }
    // Descent's SPPG -- but for fp32 gradient rows of 16 vectors (D = 64), whose MODE 1 kernel spilt 2 registers
    // at SPPG = 8 with the Philox rounds at the write: half as many there (as the split rule)
    template <typename G> static constexpr int singles_ppg() { return fewer_singles(G::SPPG, G::NE == 4 && G::LPR == 16 ? 2 : 1); }
    static constexpr int scalar_threads(int D) { return D; }
    __device__ __forceinline__ void load_step() {
        const uint64_t s = ldg<uint64_t>(step);
#if defined(__HIP_DEVICE_COMPILE__)
        s0 = __builtin_amdgcn_readfirstlane((uint32_t)s);
        s1 = __builtin_amdgcn_readfirstlane((uint32_t)(s >> 32));
#else  // host pass of the device code: never executed
        s0 = (uint32_t)s;
        s1 = (uint32_t)(s >> 32);
#endif
    }
    // the store of NE (4 or 8) elements f from column c0 (a multiple of 4) of row r of table t, at dst
    template <int NE>
    __device__ __forceinline__ void store(uint16_t* dst, int t, uint32_t r, int c0, const float* f) const {
        typename Halves<NE>::type o;
#pragma unroll
        for (int k = 0; k < NE / 4; ++k) {
            uint32_t x[4] = {r, ((uint32_t)t << 16) | (uint32_t)((c0 >> 2) + k), s0, s1};
            philox4x32_10(x, k0, k1);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[k * 4 + e] = sr_bf16(f[k * 4 + e], x[e] & 0xffffu);
        }
        stg<typename Halves<NE>::type>(dst, o);
    }
    template <typename TT, typename F>
    __device__ __forceinline__ void scalar_write(TT* __restrict__ row, float*, int64_t r, int, int c, int t,
                                                 F&& colsum) const {
        static_assert(sizeof(TT) == 2, "stochastic rounding is of bf16 tables");
        const float w = __builtin_fmaf(-lr, colsum(c), to_f32(row[c]));
        uint32_t x[4] = {(uint32_t)r, ((uint32_t)t << 16) | (uint32_t)(c >> 2), s0, s1};
        philox4x32_10(x, k0, k1);
        stg<uint16_t>(row + c, sr_bf16(w, x[c & 3] & 0xffffu));
    }
};
// ---- the Adagrad rules with the stochastic store (bf16 tables): G, the state update and the fp32 result W' of every
// element are the parent rule's at that write site (the same expressions in the same order: the items branch on the
// parent's kState), the state is written with the parent's bits, and the element stored is sr_bf16(W', R) with the
// R, the key and the counter defined above.  A rule is its parent's fields and SrWord: the seed's halves, the handle's
// step word and its value; the word is read and advanced as StochasticDescent's is.
struct SrWord {
    uint32_t k0, k1;       // the seed's halves
    const uint64_t* step;  // the handle's step word
    uint32_t s0, s1;       // its value, by load_step
    static constexpr bool kRederiveLane = true;  // (rederives_lane, below)
    __device__ __forceinline__ void load_step() {
        const uint64_t s = ldg<uint64_t>(step);
#if defined(__HIP_DEVICE_COMPILE__)
        s0 = __builtin_amdgcn_readfirstlane((uint32_t)s);
        s1 = __builtin_amdgcn_readfirstlane((uint32_t)(s >> 32));
#else  // host pass of the device code: never executed
        s0 = (uint32_t)s;
        s1 = (uint32_t)(s >> 32);
#endif
    }
    // the output block of columns 4b .. 4b + 3 of row r of table t
    __device__ __forceinline__ void block(uint32_t* x, int t, uint32_t r, int b) const {
        x[0] = r;
        x[1] = ((uint32_t)t << 16) | (uint32_t)b;
        x[2] = s0;
        x[3] = s1;
        // the ten round keys are made here, at the write: left to the compiler they are hoisted out of the item loop
        // into twenty scalar registers, which these kernels (at the scalar and the 168-vector-register limits beside a
        // state stream) then spill
        uint32_t ka = k0, kb = k1;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(ka), "+s"(kb));
#endif
        philox4x32_10(x, ka, kb);
    }
    // column c's 16 bits of its block x (by selects: a variable index would put x in scratch)
    __device__ static __forceinline__ uint32_t bits_of(const uint32_t* x, int c) {
        const uint32_t lo = (c & 1) ? x[1] : x[0], hi = (c & 1) ? x[3] : x[2];
        return ((c & 2) ? hi : lo) & 0xffffu;
    }
    // the store of NE (4 or 8) elements f from column c0 (a multiple of 4) of row r of table t, at dst
    template <int NE>
    __device__ __forceinline__ void store(uint16_t* dst, int t, uint32_t r, int c0, const float* f) const {
        typename Halves<NE>::type o;
#pragma unroll
        for (int k = 0; k < NE / 4; ++k) {
            uint32_t x[4];
            block(x, t, r, (c0 >> 2) + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[k * 4 + e] = sr_bf16(f[k * 4 + e], x[e] & 0xffffu);
        }
        stg<typename Halves<NE>::type>(dst, o);
    }
};

struct StochasticAdagrad : Adagrad, SrWord {
    static constexpr bool kStochastic = true;
    // MODE >= 2 over the training step's fp32 dt, in a unit of its own (sr_adagrad_step.hip), so sr_adagrad.hip stays
    // the MODE 0 / 1 unit it was
    static constexpr bool kCarriesBuild = true;
    static constexpr bool kBuildWithApply = false;
    static constexpr bool kF32Tables = false;     // fp32 tables: nothing to round
    // the parent's count (the Philox rounds come at the write, after the loads) -- but for fp32 gradient rows of 16
    // vectors (D = 64), whose MODE 1 kernel spilt 2 registers with it: half as many there (as StochasticDescent)
    template <typename G> static constexpr int singles_ppg() {
        return fewer_singles(Adagrad::template singles_ppg<G>(), G::NE == 4 && G::LPR == 16 ? 2 : 1);
    }
    template <typename TT, typename F>
    __device__ __forceinline__ void scalar_write(TT* __restrict__ row, float* __restrict__ st, int64_t r, int D, int c, int t,
                                                 F&& colsum) const {
        static_assert(sizeof(TT) == 2, "stochastic rounding is of bf16 tables");
        const float g = colsum(c);
        float a = st[r * D + c], w = to_f32(row[c]);
        adagrad_step<1>(lr, eps, &g, &a, &w);
        st[r * D + c] = a;
        uint32_t x[4];
        block(x, t, (uint32_t)r, c >> 2);
        stg<uint16_t>((uint16_t*)row + c, sr_bf16(w, bits_of(x, c)));
    }
};

struct StochasticRowwiseAdagrad : RowwiseAdagrad, SrWord {
    static constexpr bool kStochastic = true;
    static constexpr bool kCarriesBuild = true;  // (sr_adagrad_rowwise_step.hip, as StochasticAdagrad)
    static constexpr bool kBuildWithApply = false;
    static constexpr bool kF32Tables = false;
    // (the parent's count, and half of it for fp32 gradient rows of 16 vectors: as StochasticAdagrad)
    template <typename G> static constexpr int singles_ppg() {
        return fewer_singles(RowwiseAdagrad::template singles_ppg<G>(), G::NE == 4 && G::LPR == 16 ? 2 : 1);
    }
    // (c = 0: the thread has the whole row; the squares in column order, then the step, a block per four columns)
    template <typename TT, typename F>
    __device__ __forceinline__ void scalar_write(TT* __restrict__ row, float* __restrict__ st, int64_t r, int D, int, int t,
                                                 F&& colsum) const {
        static_assert(sizeof(TT) == 2, "stochastic rounding is of bf16 tables");
        float ss = 0.0f;
        for (int k = 0; k < D; ++k) {
            const float g = colsum(k);
            ss = __builtin_fmaf(g, g, ss);
        }
        const float m = rowwise_m(st[r], ss, D);
        const float s = rowwise_scale(lr, eps, m);
        st[r] = m;
        uint32_t x[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k < D; ++k) {
            if ((k & 3) == 0) block(x, t, (uint32_t)r, k >> 2);
            const float w = __builtin_fmaf(-s, colsum(k), to_f32(row[k]));
            stg<uint16_t>((uint16_t*)row + k, sr_bf16(w, bits_of(x, k)));
        }
    }
};

// Whether the apply kernel makes a lane's group constants again in every chunk and once-hit item (R::kRederiveLane):
// the stochastic Adagrad rules, whose kernels hold a state stream and the Philox rounds under the 168 registers of
// three workgroups per CU, and spilt two loop-invariant registers without it.  Every other rule: no, and its kernels
// are what they were.
template <typename R, typename = void> struct rederives_lane { static constexpr bool value = false; };
template <typename R> struct rederives_lane<R, decltype((void)R::kRederiveLane)> { static constexpr bool value = R::kRederiveLane; };

// a rule's write of NE weights f at column c0 of row r (at `row`) of table t
template <typename TT, int NE, typename R>
__device__ __forceinline__ void rule_store(const R& rule, TT* row, int t, uint32_t r, int c0, const float* f) {
    if constexpr (R::kStochastic) {
        static_assert(sizeof(TT) == 2, "stochastic rounding is of bf16 tables");
        rule.template store<NE>((uint16_t*)row + c0, t, r, c0, f);
    } else {
        store_row<TT, NE>(row, c0, f);
    }
}

// ---- a chunk, by one lane group (lane v of LPR; gl0 = the group's first lane in the wave; t = the table)
template <typename TT, typename GT, int VPR, typename R>
__device__ __forceinline__ void run_chunk(const int32_t* __restrict__ perm, const int4& a, const int4& b,
                                          TT* __restrict__ table, typename R::State* __restrict__ st,
                                          const GT* __restrict__ gbase, int64_t grad_ld, const FastDiv& L,
                                          const R& rule, int v, int gl0, int t) {
    typedef ApplyGeom<GT, VPR> G;
    constexpr int NE = G::NE, D = G::D, LPR = G::LPR;
    constexpr int KX = (kChunk - kChunkInline + LPR - 1) / LPR;  // perm loads per lane (long chunks)
    const int beg = a.x, len = a.y - a.x;
    TT* row = table + (int64_t)(uint32_t)a.z * D;
    float tv[G::VPL][NE];
    typename Halves<NE>::type hv[G::VPL], lv[G::VPL];  // split: the row's halves, as bits
    if constexpr (R::kState == 3) {
        static_assert(sizeof(TT) == 2, "split rows live in bf16 tables");
#pragma unroll
        for (int j = 0; j < G::VPL; ++j) {
            hv[j] = load_halves<NE>((const uint16_t*)row + (v + j * 64) * NE);
            lv[j] = load_halves<NE>(st + (int64_t)(uint32_t)a.z * D + (v + j * 64) * NE);
        }
    } else {
#pragma unroll
        for (int j = 0; j < G::VPL; ++j) load_row<TT, NE>(row, (v + j * 64) * NE, tv[j]);  // beside the grad rows
    }
    float sv[R::kState == 1 ? G::VPL : 1][NE];  // Adagrad: the state row
    float m = 0.0f;                             // row-wise: the state word
    if constexpr (R::kState == 1) {
#pragma unroll
        for (int j = 0; j < G::VPL; ++j) load_row<float, NE>(st + (int64_t)(uint32_t)a.z * D, (v + j * 64) * NE, sv[j]);
    }
    if constexpr (R::kState == 2) m = ldg<float>(st + (uint32_t)a.z);
    const int inl[kChunkInline] = {a.w, b.x, b.y, b.z, b.w};
    int px[KX];  // positions kChunkInline.. : position kChunkInline + k*LPR + lane
    if (len > kChunkInline) {
#pragma unroll
        for (int k = 0; k < KX; ++k) {
            const int u = kChunkInline + k * LPR + v;
            px[k] = u < len ? perm[beg + u] : 0;
        }
    }
    float acc[G::VPL][NE];
#pragma unroll
    for (int j = 0; j < G::VPL; ++j)
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[j][e] = 0.0f;
    constexpr int IF = G::IF;
#pragma unroll
    for (int u0 = 0; u0 < kChunk; u0 += IF) {
        if (u0 >= len) break;  // uniform over the group
        typename Vec<GT>::type gv[IF][G::VPL];
#pragma unroll
        for (int uu = 0; uu < IF; ++uu) {
            const int u = u0 + uu;
            if (u < len) {
                const int p = u < kChunkInline ? inl[u < kChunkInline ? u : 0]
                                               : __shfl(px[(u - kChunkInline) / LPR], gl0 + (u - kChunkInline) % LPR, 64);
#pragma unroll
                for (int j = 0; j < G::VPL; ++j) gv[uu][j] = grad_vec<GT>(gbase, grad_ld, L, p, v + j * 64);
            }
        }
#pragma unroll
        for (int uu = 0; uu < IF; ++uu)
            if (u0 + uu < len)
#pragma unroll
                for (int j = 0; j < G::VPL; ++j) add_vec<GT>(acc[j], gv[uu][j]);
    }
    if constexpr (R::kState == 1) {
#pragma unroll
        for (int j = 0; j < G::VPL; ++j) {
            adagrad_step<NE>(rule.lr, rule.eps, acc[j], sv[j], tv[j]);
            store_row<float, NE>(st + (int64_t)(uint32_t)a.z * D, (v + j * 64) * NE, sv[j]);
            rule_store<TT, NE>(rule, row, t, (uint32_t)a.z, (v + j * 64) * NE, tv[j]);
        }
        return;
    }
    if constexpr (R::kState == 3) {
#pragma unroll
        for (int j = 0; j < G::VPL; ++j)
            split_write<NE>(rule.lr, acc[j], hv[j], lv[j], (uint16_t*)row + (v + j * 64) * NE,
                            st + (int64_t)(uint32_t)a.z * D + (v + j * 64) * NE);
        return;
    }
    float lr = rule.lr;
    if constexpr (R::kState == 2) {
        float ss = 0.0f;
#pragma unroll
        for (int j = 0; j < G::VPL; ++j) ss = sum_squares<NE>(acc[j], ss);
#pragma unroll
        for (int o = 1; o < LPR; o <<= 1) ss += __shfl_xor(ss, o, 64);
        m = rowwise_m(m, ss, D);
        lr = rowwise_scale(rule.lr, rule.eps, m);
        if (v == 0) stg<float>(st + (uint32_t)a.z, m);
    }
#pragma unroll
    for (int j = 0; j < G::VPL; ++j) {
#pragma unroll
        for (int e = 0; e < NE; ++e) tv[j][e] = __builtin_fmaf(-lr, acc[j][e], tv[j][e]);
        rule_store<TT, NE>(rule, row, t, (uint32_t)a.z, (v + j * 64) * NE, tv[j]);
    }
}

// ---- once-hit positions of a split indexer (single[p] = 1: the position's row is hit by no other
// position), SPPG consecutive positions per lane group: w = fmaf(-lr, 0 + g, w), the chunk
// path's arithmetic for a one-position segment, with no descriptor or perm read.
struct SinglesArgs {
    const uint8_t* single;  // [T][cap] (IndexerDev::single); NULL: no singles items
    const void* idx;
    int itype;
    int64_t tstride;
    int base;
    int N;                  // positions per table
};
template <typename TT, typename GT, int VPR, typename R>
__device__ __forceinline__ void run_singles(const SinglesArgs& sa, int64_t cap, TT* __restrict__ table,
                                            typename R::State* __restrict__ st, int64_t nrows, int t, int p0,
                                            const GT* __restrict__ gbase, int64_t grad_ld, const FastDiv& L,
                                            const R& rule, int v, int gl0) {
    typedef ApplyGeom<GT, VPR> G;
    constexpr int NE = G::NE, D = G::D, LPR = G::LPR, PPG = R::template singles_ppg<G>();
    constexpr int KX = (PPG + LPR - 1) / LPR;
    uint32_t pr[KX];  // the row of position p0 + k*LPR + v, ~0u when it is not a single
#pragma unroll
    for (int k = 0; k < KX; ++k) {
        const int u = k * LPR + v;
        const bool ok = u < PPG && p0 + u < sa.N;
        const uint8_t fl = ok ? ldg<uint8_t>(sa.single + (int64_t)t * cap + p0 + u) : (uint8_t)0;
        const int64_t r = load_index_if(ok, sa.idx, sa.itype, (int64_t)t * sa.tstride + p0 + u) - sa.base;
        pr[k] = (fl && r >= 0 && r < nrows) ? (uint32_t)r : ~0u;
    }
    uint32_t ru[PPG];
    typename Vec<GT>::type gv[PPG][G::VPL];
    float tv[PPG][G::VPL][NE];
    float sv[R::kState == 1 ? PPG : 1][R::kState == 1 ? G::VPL : 1][NE];  // Adagrad: the state rows
    float m[PPG];                                                         // row-wise: the state words
    typename Halves<NE>::type hv[PPG][G::VPL], lv[PPG][G::VPL];           // split: the rows' halves, as bits
#pragma unroll
    for (int u = 0; u < PPG; ++u) {
        ru[u] = (uint32_t)__shfl((int)pr[u / LPR], gl0 + u % LPR, 64);
        if (ru[u] != ~0u) {
#pragma unroll
            for (int j = 0; j < G::VPL; ++j) {
                gv[u][j] = grad_vec<GT>(gbase, grad_ld, L, p0 + u, v + j * 64);
                if constexpr (R::kState == 3) {
                    hv[u][j] = load_halves<NE>((const uint16_t*)table + (int64_t)ru[u] * D + (v + j * 64) * NE);
                    lv[u][j] = load_halves<NE>(st + (int64_t)ru[u] * D + (v + j * 64) * NE);
                } else {
                    load_row<TT, NE>(table + (int64_t)ru[u] * D, (v + j * 64) * NE, tv[u][j]);
                }
                if constexpr (R::kState == 1) load_row<float, NE>(st + (int64_t)ru[u] * D, (v + j * 64) * NE, sv[u][j]);
            }
            if constexpr (R::kState == 2) m[u] = ldg<float>(st + ru[u]);
        }
    }
    if constexpr (R::kState != 0) {
#pragma unroll
        for (int u = 0; u < PPG; ++u)
            if (ru[u] != ~0u) {  // (uniform over the lane group)
                float g[G::VPL][NE];
#pragma unroll
                for (int j = 0; j < G::VPL; ++j) {
                    Vec<GT>::to_f32(gv[u][j], g[j]);
#pragma unroll
                    for (int e = 0; e < NE; ++e) g[j][e] = 0.0f + g[j][e];
                }
                float lr = rule.lr;
                if constexpr (R::kState == 2) {
                    float ss = 0.0f;
#pragma unroll
                    for (int j = 0; j < G::VPL; ++j) ss = sum_squares<NE>(g[j], ss);
#pragma unroll
                    for (int o = 1; o < LPR; o <<= 1) ss += __shfl_xor(ss, o, 64);
                    m[u] = rowwise_m(m[u], ss, D);
                    lr = rowwise_scale(rule.lr, rule.eps, m[u]);
                    if (v == 0) stg<float>(st + ru[u], m[u]);
                }
#pragma unroll
                for (int j = 0; j < G::VPL; ++j) {
                    if constexpr (R::kState == 3) {
                        split_write<NE>(rule.lr, g[j], hv[u][j], lv[u][j],
                                        (uint16_t*)table + (int64_t)ru[u] * D + (v + j * 64) * NE,
                                        st + (int64_t)ru[u] * D + (v + j * 64) * NE);
                    } else {
                        if constexpr (R::kState == 1) {
                            adagrad_step<NE>(rule.lr, rule.eps, g[j], sv[u][j], tv[u][j]);
                            store_row<float, NE>(st + (int64_t)ru[u] * D, (v + j * 64) * NE, sv[u][j]);
                        } else {
#pragma unroll
                            for (int e = 0; e < NE; ++e) tv[u][j][e] = __builtin_fmaf(-lr, g[j][e], tv[u][j][e]);
                        }
                        rule_store<TT, NE>(rule, table + (int64_t)ru[u] * D, t, ru[u], (v + j * 64) * NE, tv[u][j]);
                    }
                }
            }
        return;
    }
    const float lr = rule.lr;
#pragma unroll
    for (int u = 0; u < PPG; ++u)
        if (ru[u] != ~0u)
#pragma unroll
            for (int j = 0; j < G::VPL; ++j) {
                float g[NE];
                Vec<GT>::to_f32(gv[u][j], g);
#pragma unroll
                for (int e = 0; e < NE; ++e) tv[u][j][e] = __builtin_fmaf(-lr, 0.0f + g[e], tv[u][j][e]);
                store_row<TT, NE>(table + (int64_t)ru[u] * D, (v + j * 64) * NE, tv[u][j]);
            }
}

// The NEXT batch's split indexer, built by extra workgroups of this apply launch (the training
// step's pipelined form: dlrm_step_bwd_prepare).  Its bounds errors go to `err` (private: the next
// step's forward gathers the same indices and raises them on the context's flag).
struct PrepArgs {
    IndexerDev ix;
    const TableDesc* tabs;  // the tables (for nrows)
    int T;                  // real tables
    const void* idx;
    int itype;
    int64_t tstride;
    int base;
    int N;
    unsigned* err;
};

// LDS of a hot-slice item (one workgroup)
template <int D>
struct SliceLds {
    f32x4 wsum[kApplyWaves][D / 4];   // per-wave partial rows
    int last;
};

// ---- a slice of a hot segment, by the whole workgroup: pos = its positions (perm entries),
// len of them, `row` the table row, `ns` the slices of its segment, its partial row at
// part_me, the segment's first at part_first (slot spacing pdim), `cnt` the segment's arrival
// counter (zero at rest); (t, r) = the table and the row's index, for a rule whose store depends on them.
// The row's write by the first D/4 threads (row r of table t; G = the thread's four sums, rw its four weights, sw its
// four accumulators or the row's word); every thread of the workgroup calls it.  wsum_read: other
// waves may still be reading sm.wsum (the row-wise wave totals of D > 256 reuse it).
// (The split rule: rh / rl = the thread's four high and low halves, as bits, in place of rw / sw.)
template <typename TT, typename R, int D>
__device__ __forceinline__ void slice_write(const R& rule, const f32x4& G, float* rw, float* sw, u16x4& rh, u16x4& rl,
                                            TT* __restrict__ row, typename R::State* __restrict__ srow, SliceLds<D>& sm,
                                            bool wsum_read, int t, uint32_t r) {
    const int tid = threadIdx.x;
    const bool mine = tid < D / 4;
    const float g[4] = {G[0], G[1], G[2], G[3]};
    float lr = rule.lr;
    if constexpr (R::kState == 3) {
        if (mine) split_write<4>(rule.lr, g, rh, rl, (uint16_t*)row + tid * 4, srow + tid * 4);
        return;
    }
    if constexpr (R::kState == 1) {
        if (mine) {
            adagrad_step<4>(rule.lr, rule.eps, g, sw, rw);
            store_row<float, 4>(srow, tid * 4, sw);
            rule_store<TT, 4>(rule, row, t, r, tid * 4, rw);
        }
        return;
    }
    if constexpr (R::kState == 2) {
        float ss = mine ? sum_squares<4>(g, 0.0f) : 0.0f;  // (lanes past the row add 0)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) ss += __shfl_xor(ss, o, 64);
        if constexpr (D / 4 > 64) {  // the wave totals, in wave order
            if (wsum_read) __syncthreads();
            float* wt = (float*)&sm.wsum[0][0];
            if ((tid & 63) == 0) wt[tid >> 6] = ss;
            __syncthreads();
            ss = 0.0f;
#pragma unroll
            for (int ww = 0; ww < kApplyWaves; ++ww) ss += wt[ww];
        }
        const float m = rowwise_m(sw[0], ss, D);
        lr = rowwise_scale(rule.lr, rule.eps, m);
        if (tid == 0) stg<float>(srow, m);
    }
    if (mine) {
#pragma unroll
        for (int e = 0; e < 4; ++e) rw[e] = __builtin_fmaf(-lr, g[e], rw[e]);
        rule_store<TT, 4>(rule, row, t, r, tid * 4, rw);
    }
}

template <typename TT, typename GT, int VPR, typename R>
__device__ __forceinline__ void slice_body(const int32_t* __restrict__ pos, int len, TT* __restrict__ row,
                                           typename R::State* __restrict__ srow, int ns, float* part_me, const float* part_first,
                                           int64_t pdim, int32_t* cnt_p, const GT* __restrict__ gbase, int64_t grad_ld,
                                           const FastDiv& L, const R& rule, SliceLds<ApplyGeom<GT, VPR>::D>& sm, int t,
                                           uint32_t r) {
    typedef ApplyGeom<GT, VPR> G;
    constexpr int NE = G::NE, D = G::D, LPR = G::LPR, NG = G::NG;
    constexpr int SPG = (kHotSlice + NG - 1) / NG;  // positions per lane group
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane / LPR, v = lane % LPR, gid = w * G::RPW + g;
    // the table row, loaded now (needed only at the end; no other item writes it in this launch)
    float rw[4];
    u16x4 rh = u16x4{0, 0, 0, 0}, rl = u16x4{0, 0, 0, 0};  // split: the row's halves, as bits
    if constexpr (R::kState == 3) {
        static_assert(sizeof(TT) == 2, "split rows live in bf16 tables");
        if (tid < D / 4) {
            rh = load_halves<4>((const uint16_t*)row + tid * 4);
            rl = load_halves<4>(srow + tid * 4);
        }
    } else {
        if (tid < D / 4) load_row<TT, 4>(row, tid * 4, rw);
    }
    float sw[4] = {0.f, 0.f, 0.f, 0.f};  // the state, with the row (written by the segment's last slice only)
    if constexpr (R::kState == 1) {
        if (tid < D / 4) load_row<float, 4>(srow, tid * 4, sw);
    }
    if constexpr (R::kState == 2) {
        if (tid < D / 4) sw[0] = ldg<float>(srow);
    }
    // this group's consecutive share [g0, u1), in position order: lane v of the group loads
    // positions g0 + k LPR + v, and each row's position comes by a shuffle (no LDS staging and no
    // barrier before the grad rows)
    const int g0 = gid * SPG, u1 = min(len, g0 + SPG);  // (SPG = kHotSlice / NG)
    static_assert(SPG <= LPR, "one position per lane of the group");
    const int gl0 = lane - v;
    const int px = g0 + v < u1 ? pos[g0 + v] : 0;
    float acc[G::VPL][NE];
#pragma unroll
    for (int j = 0; j < G::VPL; ++j)
#pragma unroll
        for (int e = 0; e < NE; ++e) acc[j][e] = 0.0f;
    // grad rows in flight per lane: a lane group's whole share at one 16-B vector per row
    // up to kSliceIF, else the chunk items' IF
    constexpr int IFS = G::VPL == 1 ? (SPG < G::SIF ? SPG : G::SIF) : G::IF;
    constexpr int IF = IFS < SPG ? IFS : SPG;
#pragma unroll 1
    for (int r0 = 0; r0 < SPG; r0 += IF) {
        const int u0 = g0 + r0;
        if (u0 >= u1) break;  // uniform over the group
        typename Vec<GT>::type gv[IF][G::VPL];
#pragma unroll
        for (int uu = 0; uu < IF; ++uu) {
            const int p = __shfl(px, gl0 + r0 + uu, 64);
            if (u0 + uu < u1)
#pragma unroll
                for (int j = 0; j < G::VPL; ++j) gv[uu][j] = grad_vec<GT>(gbase, grad_ld, L, p, v + j * 64);
        }
#pragma unroll
        for (int uu = 0; uu < IF; ++uu)
            if (u0 + uu < u1)
#pragma unroll
                for (int j = 0; j < G::VPL; ++j) add_vec<GT>(acc[j], gv[uu][j]);
    }
    // the wave's groups: xor butterfly over the group bits of the lane (fixed order)
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
        for (int j = 0; j < G::VPL; ++j)
#pragma unroll
            for (int e = 0; e < NE; ++e) acc[j][e] += __shfl_xor(acc[j][e], o, 64);
    if (g == 0)
#pragma unroll
        for (int j = 0; j < G::VPL; ++j)
#pragma unroll
            for (int e = 0; e < NE; e += 4)
                sm.wsum[w][((v + j * 64) * NE + e) / 4] = f32x4{acc[j][e], acc[j][e + 1], acc[j][e + 2], acc[j][e + 3]};
    __syncthreads();
    // the waves, in wave order, by the first D/4 threads (one float4 of the row each)
    f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
    if (tid < D / 4) {
#pragma unroll
        for (int ww = 0; ww < kApplyWaves; ++ww) sum += sm.wsum[ww][tid];
    }
    static_assert(D / 4 <= kApplyThreads, "a float4 of the row per thread");
    if (ns == 1) {
        if constexpr (R::kState == 0) {
            const float lr = rule.lr;
            if (tid < D / 4) {
#pragma unroll
                for (int e = 0; e < 4; ++e) rw[e] = __builtin_fmaf(-lr, sum[e], rw[e]);
                store_row<TT, 4>(row, tid * 4, rw);
            }
        } else {
            slice_write<TT, R, D>(rule, sum, rw, sw, rh, rl, row, srow, sm, true, t, r);
        }
        __syncthreads();  // sm reused by this workgroup's next item
        return;
    }
    gi32_t* cnt = (gi32_t*)cnt_p;
    if (tid < D / 4) store_sc1(part_me + tid * 4, sum);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains before the arrival
    if (D / 4 > 64) __syncthreads();                   // (several storing waves)
    if (tid == 0) sm.last = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ns - 1;
    __syncthreads();
    if constexpr (R::kState == 0) {
        const float lr = rule.lr;
        if (sm.last && tid < D / 4) {
            float* f = rw;
            const float* first = part_first + tid * 4;
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
            constexpr int PB = 16;  // partial rows in flight
            for (int k0 = 0; k0 < ns; k0 += PB) {
                f32x4 q[PB];
#pragma unroll
                for (int u = 0; u < PB; ++u) q[u] = load_sc1(first + (int64_t)(k0 + u < ns ? k0 + u : k0) * pdim);
#pragma unroll
                for (int u = 0; u < PB; ++u)
                    if (k0 + u < ns) s += q[u];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = __builtin_fmaf(-lr, s[e], f[e]);
            store_row<TT, 4>(row, tid * 4, f);
            if (tid == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else if (sm.last) {  // (uniform over the workgroup: the row-wise reduction has barriers)
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
        if (tid < D / 4) {
            const float* first = part_first + tid * 4;
            constexpr int PB = 16;  // partial rows in flight
            for (int k0 = 0; k0 < ns; k0 += PB) {
                f32x4 q[PB];
#pragma unroll
                for (int u = 0; u < PB; ++u) q[u] = load_sc1(first + (int64_t)(k0 + u < ns ? k0 + u : k0) * pdim);
#pragma unroll
                for (int u = 0; u < PB; ++u)
                    if (k0 + u < ns) s += q[u];
            }
        }
        slice_write<TT, R, D>(rule, s, rw, sw, rh, rl, row, srow, sm, false, t, r);  // (sm.wsum: read before the barriers above)
        if (tid == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();  // sm reused by this workgroup's next item
}

// ---- a slice of a hot segment located by (virtual table vt, local slice sl): sd = {p0, p1,
// row, h}; the segment's descriptor ix.hot[vt][h] = {beg, end, row, first slice}
template <typename TT, typename GT, int VPR, typename R>
__device__ __forceinline__ void run_slice(const IndexerDev& ix, int vt, int sl, const int4& sd, TT* __restrict__ table,
                                          typename R::State* __restrict__ st, const GT* __restrict__ gbase, int64_t grad_ld,
                                          const FastDiv& L, const R& rule, SliceLds<ApplyGeom<GT, VPR>::D>& sm, int t) {
    constexpr int D = ApplyGeom<GT, VPR>::D;
    const int64_t off = (int64_t)vt * ix.cap;
    const int4 hd = ix.hot[off + sd.w];
    const int ns = (hd.y - hd.x + kHotSlice - 1) / kHotSlice;
    float* pbase = ix.partial + (int64_t)vt * ix.pcap * ix.pdim;
    slice_body<TT, GT, VPR, R>(ix.perm + off + sd.x, sd.y - sd.x, table + (int64_t)(uint32_t)sd.z * D,
                               R::template state_row<D>(st, (uint32_t)sd.z), ns, pbase + (int64_t)sl * ix.pdim,
                               pbase + (int64_t)hd.w * ix.pdim, ix.pdim, ix.hot_cnt + off + sd.w, gbase, grad_ld, L,
                               rule, sm, t, (uint32_t)sd.z);
}

// ---- hot slice k of the item map (one 32-B record: IndexerDev::slice_rec); k and its segment's
// first slice `first` count over the sub-lists' slices in order (partial row and counter slots)
template <typename TT, typename GT, int VPR, typename R>
__device__ __forceinline__ void run_slice_rec(const IndexerDev& ix, int k, int first, const int4& r0, const int4& r1,
                                              TT* __restrict__ table, typename R::State* __restrict__ st,
                                              const GT* __restrict__ gbase, int64_t grad_ld, const FastDiv& L,
                                              const R& rule, SliceLds<ApplyGeom<GT, VPR>::D>& sm, int t) {
    constexpr int D = ApplyGeom<GT, VPR>::D;
    slice_body<TT, GT, VPR, R>(ix.perm + r0.x, r0.y - r0.x, table + (int64_t)(uint32_t)r0.z * D,
                               R::template state_row<D>(st, (uint32_t)r0.z), r1.x, ix.partial + (int64_t)k * ix.pdim,
                               ix.partial + (int64_t)first * ix.pdim, ix.pdim, ix.hot_cnt + first, gbase, grad_ld, L,
                               rule, sm, t, (uint32_t)r0.z);
}

}  // namespace dlrm
