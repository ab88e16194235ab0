// apply_kernel.hpp -- the apply launch of update! (sgd_apply_kernel over apply.hpp's work items), its
// any-D fallback kernels and their launchers, by update rule.  update.hip instantiates Descent
// (every MODE), adagrad.hip and adagrad_rowwise.hip the Adagrad rules, split_sgd.hip the split rule and sr_sgd.hip
// the stochastic rule (MODE 0 and 1), and split_step.hip, adagrad_step.hip, adagrad_rowwise_step.hip and sr_step.hip those four
// rules' build-carrying launches (MODE 2 / 3 / 5), and sr_adagrad.hip and sr_adagrad_rowwise.hip the Adagrad rules with the
// stochastic store (MODE 0 and 1): they compile side by side.
#pragma once
#include "apply.hpp"

#ifndef ITEM_START  // (update.hip's profiling variant defines these before the include)
#define ITEM_START(kind, k, item) do {} while (0)
#define ITEM_END(k) do {} while (0)
#define APPLY_START(kind) do {} while (0)
#define APPLY_END() do {} while (0)
#endif

namespace dlrm {

// step_index_kernel's own launch (update.hip): the next batch's split build when the apply launch
// cannot carry it
void launch_step_index(hipStream_t s, const PrepArgs& pa);

// ------------------------------------------------------------------------------ apply
// Persistent launch, flat over tables (apply.hpp).  Work items: [0, S) = the S slices of every
// table's hot segments (one workgroup each, handed out first: the longest chains), then
// ceil(C / NG) items of NG chunks (one per lane group), then (singles: a split indexer whose
// once-hit rows are this launch's too) T * ceil(N / (NG * SPPG)) items of once-hit
// positions.  Workgroup b takes items b, b + grid, ...: every item is short, so static striding
// balances, and no workgroup is launched past the work.
// MODE 0: chunks + hot slices; 1: + once-hit (singles) items; 2: + the next batch's split indexer
// in the first (pa.T << pa.ix.vshift) / 4 workgroups (PrepArgs); 3: the same for more than 2048
// positions per table in rounds; 5: the same by the scan build.
#ifndef DLRM_BUILD_PRIO
#define DLRM_BUILD_PRIO 3
#endif
constexpr int kBuildPrio = DLRM_BUILD_PRIO;  // s_setprio of the in-apply build's waves (0..3)

// The wave build's kernel for the build `pa` (build_plan.hpp wave_kind): one round up to 2048 positions per
// table; above, the scan build (indexer.hpp wave_build_group_scan; int32 indices, 16-B aligned per table,
// N % 4 == 0), the default, or rounds (wave_build_group<true>, any index type; DLRM_WAVE_ROUNDS=1 forces it).
// PrepArgs is a kernel argument and cannot carry the plan's answer, so the two launchers that take one ask here.
static inline int prep_wave_kind(const PrepArgs& pa) {
    return wave_kind(pa.N, idx_vec32(pa.idx, pa.itype, pa.tstride), knobs());
}
// workgroups of a build (4 parts each)
__host__ __device__ __forceinline__ int prep_groups(const PrepArgs& pa) { return (pa.T << pa.ix.vshift) / kWaveParts; }

// An item's place by the scan of the tables' counts (indexer.hpp locate).  A rule at the register limit (apply.hpp
// rederives_lane) reads the counts through an opaque copy of their address, so the lane's address into them (the walk
// over more than 256 tables) is made in the item, not held across the item loop.
template <typename R>
__device__ __forceinline__ void locate_item(const IndexerDev& ix, int T_, int which, const TableScan& sc, int id, int& table,
                                            int& local) {
    if constexpr (rederives_lane<R>::value) {
        IndexerDev ixi = ix;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(ixi.counts));
#endif
        locate(ixi, T_, which, sc, id, table, local);
    } else {
        locate(ix, T_, which, sc, id, table, local);
    }
}

// R: the update rule (apply.hpp: Descent, Adagrad, RowwiseAdagrad, SplitDescent, StochasticDescent and the two
// stochastic Adagrad rules).
template <typename TT, typename GT, int VPR, int MODE, typename R = Descent>
__global__ __launch_bounds__(kApplyThreads, 3) void sgd_apply_kernel(IndexerDev ix, TableDesc* __restrict__ tabs, int T_,
                                                                  int L, const GT* __restrict__ grad, int64_t grad_ld,
                                                                  int64_t grad_offset, R rule,
                                                                  const unsigned* __restrict__ err, SinglesArgs sa,
                                                                  PrepArgs pa) {
    static_assert(R::kCarriesBuild || MODE <= 1, "the next batch's build rides on the launches of a rule that carries it");
    constexpr bool SG = MODE == 1;
    int bid = blockIdx.x, nblk = gridDim.x;
    if constexpr (MODE >= 2) {
        extern __shared__ __attribute__((aligned(16))) unsigned char prep_lds[];
        const int NI = prep_groups(pa);
        if (bid < NI) {  // the next batch's split build: one wave per table part (indexer.hpp)
            // the build's waves first at the issue arbiter: its chain of dependent LDS / VALU steps is
            // the launch's longest, the apply waves beside it mostly wait on memory (A/B on one box:
            // 54.72 / 54.77 -> 54.91 / 55.04 M samples/s, apply 10.58 -> 10.45 us)
            __builtin_amdgcn_s_setprio(kBuildPrio);
            ITEM_START(4, 0, bid);
            // (MODE 3 / 5: the builds of more than 2048 positions per table, in their own
            // instantiations, so the step's MODE 2 kernel keeps its registers)
            if constexpr (MODE == 5)
                wave_build_group_scan<kWaveParts>(pa.ix, bid, pa.T, pa.tabs, pa.idx, pa.tstride, pa.base, pa.N, pa.err,
                                      *(WaveBuildLds*)prep_lds);
            else
                wave_build_group<MODE == 3>(pa.ix, bid, pa.T, pa.tabs, pa.idx, pa.itype, pa.tstride, pa.base,
                                            pa.N, pa.err, *(WaveBuildLds*)prep_lds);
            ITEM_END(0);
            return;
        }
        bid -= NI;
        nblk -= NI;
#ifdef DLRM_PREP_ONLY  // (probe: the build alone in this launch)
        return;
#endif
    }
    if constexpr (R::kStochastic) rule.load_step();  // (the stochastic rule's step word, once per workgroup)
    // a bounds error raised since the last dlrm_check_bounds (the lookup or the indexer build of
    // this step): the reference's gather throws before update!, so no table row is written.  (The
    // error word is loaded with the item counts, one round trip for both.)
    const FastDiv Ld(L);  // position -> bag
    unsigned err0 = ldg<unsigned>(err);
    if (ix.build_err) {  // a standalone prepared build's out-of-range indices (written by an earlier launch)
        const unsigned be = ldg<unsigned>(ix.build_err);
        if (be && !err0 && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) raise_index_error((unsigned*)err);
        err0 |= be;
    }
    typedef ApplyGeom<GT, VPR> G;
    constexpr int D = G::D, NG = G::NG;
    __shared__ SliceLds<D> sm;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane / G::LPR, v = lane % G::LPR;
    const int gid = w * G::RPW + g;
    // where this launch's items are: the wave build's flat item map (one load per item), else a
    // wave scan of every virtual table's counts (TableScan) and a lookup in it per item
    const bool mp = ix.has_map != 0;
    TableScan sS{}, sC{};
    int Stot, Ctot;
    // the item map's sub-list counts (indexer.hpp kResLists), kept in LDS: item_tot[0..8) slices,
    // [8..16) chunks
    __shared__ int lcnt[2 * kResLists];
    const int* ls = lcnt;
    const int* lc = lcnt + kResLists;
    int lstride = 0;
    if (mp) {
        if (threadIdx.x < 2 * kResLists) lcnt[threadIdx.x] = ix.item_tot[threadIdx.x];
        __syncthreads();
        Stot = 0;
        Ctot = 0;
#pragma unroll
        for (int j = 0; j < kResLists; ++j) {
            Stot += ls[j];
            Ctot += lc[j];
        }
        lstride = res_stride(T_ / kWaveParts, ix.cap, ix.vshift);
    } else {
        sS = scan_counts(ix, T_, CNT_S);
        sC = scan_counts(ix, T_, CNT_C);
        Stot = sS.total;
        Ctot = sC.total;
    }
    if (err0) return;
    const int citems = Stot + (Ctot + NG - 1) / NG;
    constexpr int PPG = R::template singles_ppg<G>();          // once-hit positions per lane group
    constexpr int SP = NG * PPG;                               // positions per singles item
    const int per_t = SG ? (sa.N + SP - 1) / SP : 0;          // singles items per real table
    const int items = citems + (T_ >> ix.vshift) * per_t;
    // Pooled bags (L > 1): every position of a bag reads the bag's gradient row, so a table's
    // gradient slice ([B][D]: 2 MB at B = 2048, D = 256 fp32) is read about L times.  Workgroups b
    // and b + 8 share an XCD (and its L2): with the plain stride every XCD walks every table and
    // fetches each slice for itself.  Instead each XCD takes one contiguous eighth of each item
    // kind (hot slices, chunk items, once-hit items) -- about an eighth of the tables -- so a slice
    // is fetched by one L2 and re-read there.  (One-hot: each gradient row is read once; plain.)
    //   item = pos + (pos < e0 ? r0 : pos < e1 ? s1 : s2), pos = this workgroup's list position
    int pos0 = bid, step = nblk, npos = items, r0 = 0, e0 = items, s1 = 0, e1 = items, s2 = 0;
    if (L > 1 && (nblk & 7) == 0 && ((blockIdx.x - bid) & 7) == 0) {
        const int x = bid & 7, c1 = citems - Stot, c2 = items - citems;
        const int a0 = (int)((int64_t)Stot * x >> 3), b0 = (int)((int64_t)Stot * (x + 1) >> 3);
        const int a1 = (int)((int64_t)c1 * x >> 3), b1 = (int)((int64_t)c1 * (x + 1) >> 3);
        const int a2 = (int)((int64_t)c2 * x >> 3), b2 = (int)((int64_t)c2 * (x + 1) >> 3);
        r0 = a0;
        e0 = b0 - a0;
        s1 = Stot + a1 - e0;
        e1 = e0 + (b1 - a1);
        s2 = citems + a2 - e1;
        npos = e1 + (b2 - a2);
        pos0 = bid >> 3;
        step = nblk >> 3;
    }
#ifdef DLRM_PHASE
    int kk_ = 0;
#endif
    for (int pos = pos0; pos < npos; pos += step) {
        const int item = pos + (pos < e0 ? r0 : (pos < e1 ? s1 : s2));
        APPLY_START(item >= citems ? 3 : (item >= Stot ? 1 : 2));
#ifdef DLRM_PHASE
        const int k_ = kk_++;
        ITEM_START(item >= citems ? 3 : (item >= Stot ? 1 : 2), k_, item);
#undef APPLY_END
#define APPLY_END() do { ITEM_END(k_); } while (0)
#endif
        // the lane's place in its group, for the chunk and once-hit items.  A rule at the register limit (apply.hpp
        // rederives_lane) takes them through an opaque copy per item, so what is derived from them (position
        // offsets, row addresses) is made again in the item instead of being held in registers across the item loop.
        [[maybe_unused]] int vi = v, gl0 = lane - v;
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (rederives_lane<R>::value) asm volatile("" : "+v"(vi), "+v"(gl0));
#endif
        if (SG && item >= citems) {  // uniform: once-hit positions of one real table
            const int t = (item - citems) / per_t;
            const int p0 = ((item - citems) - t * per_t) * SP + gid * PPG;
            if (g >= G::RPW) continue;
            const TableDesc td = load_table(tabs, t);
            if constexpr (rederives_lane<R>::value)
                run_singles<TT, GT, VPR, R>(sa, ix.cap, (TT*)td.data, rule.base(t), td.nrows, t, p0,
                                            grad + grad_offset + (int64_t)t * D, grad_ld, Ld, rule, vi, gl0);
            else
                run_singles<TT, GT, VPR, R>(sa, ix.cap, (TT*)td.data, rule.base(t), td.nrows, t, p0,
                                            grad + grad_offset + (int64_t)t * D, grad_ld, Ld, rule, v, lane - v);
            APPLY_END();
            continue;
        }
        if (item >= Stot) {
            const int fc = (item - Stot) * NG + gid;  // flat chunk of this lane group
            const int32_t* pbase;
            int4 ca, cb;
            int t;
            if (mp) {  // the flat chunk record: perm entries global, the virtual table = beg / cap
                if (g >= G::RPW || fc >= Ctot) continue;
                const int r = res_locate(lc, fc, lstride);
                ca = ix.chunk_rec[2 * (int64_t)r];
                cb = ix.chunk_rec[2 * (int64_t)r + 1];
                pbase = ix.perm;
                t = (int)(ca.x / ix.cap);  // (the compact layout: entries of table t at [t cap, (t + 1) cap))
            } else {
                int tc, cl;
                locate_item<R>(ix, T_, CNT_C, sC, fc, tc, cl);
                if (g >= G::RPW || tc < 0) continue;
                const int64_t co = 2 * ((int64_t)tc * ix.cap + cl);
                ca = ix.chunks[co];
                cb = ix.chunks[co + 1];
                pbase = ix.perm + (int64_t)tc * ix.cap;
                t = tc >> ix.vshift;
            }
            if constexpr (rederives_lane<R>::value)
                run_chunk<TT, GT, VPR, R>(pbase, ca, cb, (TT*)tabs[t].data, rule.base(t),
                                          grad + grad_offset + (int64_t)t * D, grad_ld, Ld, rule, vi, gl0, t);
            else
                run_chunk<TT, GT, VPR, R>(pbase, ca, cb, (TT*)tabs[t].data, rule.base(t),
                                          grad + grad_offset + (int64_t)t * D, grad_ld, Ld, rule, v, lane - v, t);
            APPLY_END();
            continue;
        }
        if (mp) {  // (uniform: the slice's whole record in one 32-B load)
            const int r = res_locate(ls, item, lstride);
            const int4 r0 = ix.slice_rec[2 * (int64_t)r], r1 = ix.slice_rec[2 * (int64_t)r + 1];
            const int t = r0.w >> ix.vshift;
            run_slice_rec<TT, GT, VPR, R>(ix, item, item - (r - r1.y), r0, r1, (TT*)tabs[t].data, rule.base(t),
                                          grad + grad_offset + (int64_t)t * D, grad_ld, Ld, rule, sm, t);
            APPLY_END();
            continue;
        }
        int th, sl;
        locate_item<R>(ix, T_, CNT_S, sS, item, th, sl);  // item < S: found, the same for every lane
        const int4 sd = ix.hot_slice[(int64_t)th * ix.cap + sl];
        const int t = th >> ix.vshift;
        run_slice<TT, GT, VPR, R>(ix, th, sl, sd, (TT*)tabs[t].data, rule.base(t), grad + grad_offset + (int64_t)t * D,
                                  grad_ld, Ld, rule, sm, t);
        APPLY_END();
    }
#ifdef DLRM_PHASE
#undef APPLY_END
#define APPLY_END() do {} while (0)
#endif
}


// Generic (any D) versions: R::scalar_threads(D) threads per row (one per element column; the row-wise
// rule one per row), each calling the rule's scalar_write with colsum(c) = column c's gradient sum.
template <typename TT, typename GT, typename R>
__global__ __launch_bounds__(256) void sgd_chunks_scalar(IndexerDev ix, TableDesc* __restrict__ tabs, int D, int L,
                                                         const GT* __restrict__ grad, int64_t grad_ld,
                                                         int64_t grad_offset, R rule, const unsigned* __restrict__ err) {
    if (ix.build_err && *ix.build_err) {  // (a prepared build's bounds error: raised here, before hot / singles)
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) raise_index_error((unsigned*)err);
        return;
    }
    if (*err) return;
    if constexpr (R::kStochastic) rule.load_step();
    const int t = blockIdx.y;
    const int nchunks = ix.counts[(int64_t)t * 8 + CNT_C];
    const int64_t off = ix.part_off(t);
    const int W = R::scalar_threads(D);  // threads per row
    const int64_t total = (int64_t)nchunks * W;
    TT* table = (TT*)tabs[t >> ix.vshift].data;
    typename R::State* st = rule.base(t >> ix.vshift);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int cid = (int)(e / W);
        const int4 cd = ix.chunks[2 * (off + cid)];
        rule.scalar_write(table + (int64_t)(uint32_t)cd.z * D, st, (int64_t)(uint32_t)cd.z, D, (int)(e % W), t >> ix.vshift, [&](int c) {
            float acc = 0.0f;
            for (int i = cd.x; i < cd.y; ++i)
                acc += to_f32(grad[(int64_t)(ix.perm[off + i] / L) * grad_ld + grad_offset + (int64_t)(t >> ix.vshift) * D + c]);
            return acc;
        });
    }
}

template <typename TT, typename GT, typename R>
__global__ __launch_bounds__(256) void sgd_hot_scalar(IndexerDev ix, TableDesc* __restrict__ tabs, int D, int L,
                                                      const GT* __restrict__ grad, int64_t grad_ld,
                                                      int64_t grad_offset, R rule, const unsigned* __restrict__ err) {
    if (*err) return;
    if constexpr (R::kStochastic) rule.load_step();
    const int t = blockIdx.y;
    const int nhot = ix.counts[(int64_t)t * 8 + CNT_H];
    const int64_t off = ix.part_off(t);
    const int W = R::scalar_threads(D);  // threads per row
    const int64_t total = (int64_t)nhot * W;
    TT* table = (TT*)tabs[t >> ix.vshift].data;
    typename R::State* st = rule.base(t >> ix.vshift);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int h = (int)(e / W);
        const int4 hd = ix.hot[off + h];
        rule.scalar_write(table + (int64_t)(uint32_t)hd.z * D, st, (int64_t)(uint32_t)hd.z, D, (int)(e % W), t >> ix.vshift, [&](int c) {
            float acc = 0.0f;
            for (int i = hd.x; i < hd.y; ++i)
                acc += to_f32(grad[(int64_t)(ix.perm[off + i] / L) * grad_ld + grad_offset + (int64_t)(t >> ix.vshift) * D + c]);
            return acc;
        });
    }
}

template <typename TT, typename GT, typename R>
__global__ __launch_bounds__(256) void sgd_singles_scalar(SinglesArgs sa, int64_t cap, TableDesc* __restrict__ tabs,
                                                          int D, int L, const GT* __restrict__ grad, int64_t grad_ld,
                                                          int64_t grad_offset, R rule,
                                                          const unsigned* __restrict__ err) {
    if (*err) return;
    if constexpr (R::kStochastic) rule.load_step();
    const int t = blockIdx.y;
    const int W = R::scalar_threads(D);  // threads per position
    const int64_t total = (int64_t)sa.N * W;
    TT* table = (TT*)tabs[t].data;
    typename R::State* st = rule.base(t);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(e / W);
        if (!sa.single[(int64_t)t * cap + p]) continue;
        const int64_t r = load_index(sa.idx, sa.itype, (int64_t)t * sa.tstride + p) - sa.base;
        if (r < 0 || r >= tabs[t].nrows) continue;
        rule.scalar_write(table + r * D, st, r, D, (int)(e % W), t, [&](int c) {
            return 0.0f + to_f32(grad[(int64_t)(p / L) * grad_ld + grad_offset + (int64_t)t * D + c]);
        });
    }
}


// the apply launch that also carries the next batch's build (MODE >= 2): build workgroups first
template <typename TT, typename GT, int VPR, int MODE, typename R>
static void launch_apply_build(hipStream_t s, unsigned grid, const IndexerDev& ix, TableDesc* tabs, int T_, int L,
                               const void* grad, int64_t grad_ld, int64_t grad_offset, const R& rule,
                               const unsigned* err, const SinglesArgs& sa, const PrepArgs& pa) {
    static const hipError_t attr = hipFuncSetAttribute((const void*)sgd_apply_kernel<TT, GT, VPR, MODE, R>,
                                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       (int)sizeof(WaveBuildLds));
    (void)attr;
    hipLaunchKernelGGL((sgd_apply_kernel<TT, GT, VPR, MODE, R>), dim3(grid), dim3(kApplyThreads), sizeof(WaveBuildLds), s,
                       ix, tabs, T_, L, (const GT*)grad, grad_ld, grad_offset, rule, err, sa, pa);
}

// the persistent grid of an apply launch (T_ = virtual tables), from the occupancy of the MODE 0 kernel -- or of
// OCC, in a unit that does not hold the MODE 0 kernel
template <typename TT, typename GT, int VPR, typename R, int OCC = 0>
static int64_t apply_grid(const IndexerDev& ix, int T_, int64_t N, const SinglesArgs& sa) {
    typedef ApplyGeom<GT, VPR> G;
    // persistent grid: resident workgroups only (never more than the worst-case item count per
    // table: N / kHotSlice + N / (kChunk + 1) + 1 hot slices, N / NG chunk items, singles items)
    const int64_t SP = G::NG * R::template singles_ppg<G>();
    const int64_t ib = (int64_t)T_ * (N / kHotSlice + N / (kMinChunk + 1) + 1 + (N + G::NG - 1) / G::NG) +
                       (sa.single ? (int64_t)(T_ >> ix.vshift) * ((N + SP - 1) / SP) : 0);
    static int per_cu = 0;
    if (!per_cu) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sgd_apply_kernel<TT, GT, VPR, OCC, R>, kApplyThreads,
                                                         0) != hipSuccess || per_cu < 1)
            per_cu = 1;
    }
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    int64_t grid = (int64_t)per_cu * (cus > 0 ? cus : 256);
    if (grid > ib) grid = ib;
    if (grid < 1) grid = 1;
    return grid;
}

// ... and the launch that carries the build `pa` (no once-hit items: sa.single is NULL), by the build's size
template <typename TT, typename GT, int VPR, typename R, int OCC = 0>
static void launch_apply_build_vec(hipStream_t s, const IndexerDev& ix, TableDesc* tabs, int T_, int L, const void* grad,
                                   int64_t grad_ld, int64_t grad_offset, const R& rule, int64_t N, const unsigned* err,
                                   const SinglesArgs& sa, const PrepArgs& pa) {
    // MODE 2 + the wave build's kind: 2 one round (<= 2048 positions per table), 3 rounds, 5 scan
    const int mode = 2 + prep_wave_kind(pa);
    const unsigned g2 = (unsigned)(apply_grid<TT, GT, VPR, R, OCC>(ix, T_, N, sa) + prep_groups(pa));
    if (mode == 2) launch_apply_build<TT, GT, VPR, 2, R>(s, g2, ix, tabs, T_, L, grad, grad_ld, grad_offset, rule, err, sa, pa);
    else if (mode == 5) launch_apply_build<TT, GT, VPR, 5, R>(s, g2, ix, tabs, T_, L, grad, grad_ld, grad_offset, rule, err, sa, pa);
    else launch_apply_build<TT, GT, VPR, 3, R>(s, g2, ix, tabs, T_, L, grad, grad_ld, grad_offset, rule, err, sa, pa);
}

template <typename TT, typename GT, int VPR, typename R>
static void launch_apply_vec(hipStream_t s, const IndexerDev& ix, TableDesc* tabs, int T_, int L, const void* grad,
                             int64_t grad_ld, int64_t grad_offset, const R& rule, int64_t N, const unsigned* err,
                             const SinglesArgs& sa, const PrepArgs* pa) {
    // (the once-hit items and the next batch's indexer are separate instantiations: the step's
    // apply stays lean)
    if constexpr (R::kCarriesBuild && R::kBuildWithApply) {
        if (pa && !sa.single) {
            launch_apply_build_vec<TT, GT, VPR, R>(s, ix, tabs, T_, L, grad, grad_ld, grad_offset, rule, N, err, sa, *pa);
            return;
        }
    }
    const int64_t grid = apply_grid<TT, GT, VPR, R>(ix, T_, N, sa);
    if (sa.single)
        hipLaunchKernelGGL((sgd_apply_kernel<TT, GT, VPR, 1, R>), dim3((unsigned)grid), dim3(kApplyThreads), 0, s, ix,
                           tabs, T_, L, (const GT*)grad, grad_ld, grad_offset, rule, err, sa, PrepArgs{});
    else
        hipLaunchKernelGGL((sgd_apply_kernel<TT, GT, VPR, 0, R>), dim3((unsigned)grid), dim3(kApplyThreads), 0, s, ix,
                           tabs, T_, L, (const GT*)grad, grad_ld, grad_offset, rule, err, sa, PrepArgs{});
    // no MODE carries both once-hit items and the next batch's build: that build gets its own launch
    if (pa) launch_step_index(s, *pa);
}

template <typename TT, typename GT, typename R>
static bool dispatch_apply(int vpr, hipStream_t s, const IndexerDev& ix, TableDesc* tabs, int T_, int L,
                           const void* grad, int64_t grad_ld, int64_t grad_offset, const R& rule, int64_t N,
                           const unsigned* err, const SinglesArgs& sa, const PrepArgs* pa) {
#define DLRM_CASE(V) \
    case V: launch_apply_vec<TT, GT, V, R>(s, ix, tabs, T_, L, grad, grad_ld, grad_offset, rule, N, err, sa, pa); return true;
    switch (vpr) {
        DLRM_CASE(1) DLRM_CASE(2) DLRM_CASE(4) DLRM_CASE(8) DLRM_CASE(16) DLRM_CASE(32) DLRM_CASE(64) DLRM_CASE(128)
        default: return false;
    }
#undef DLRM_CASE
}

// f(TT(), GT()) for the table and gradient element types (a rule without kF32Tables: bf16 tables, the caller checked)
template <typename R, typename F>
static void by_dtypes(int tdtype, int gdtype, F&& f) {
    if constexpr (R::kF32Tables) {
        if (tdtype == DLRM_F32) return gdtype == DLRM_F32 ? f(float(), float()) : f(float(), uint16_t());
    }
    return gdtype == DLRM_F32 ? f(uint16_t(), float()) : f(uint16_t(), uint16_t());
}

// tabs_aligned16: every table row (and, for the element-wise Adagrad and the split rule, every state row) is
// 16-B aligned
template <typename R>
static int launch_apply_rule(dlrm_ctx* ctx, const IndexerDev& ix, TableDesc* tabs, bool tabs_aligned16, int T_, int D,
                             int tdtype, int L, int64_t N, const void* grad, int gdtype, int64_t grad_ld,
                             int64_t grad_offset, const R& rule, const SinglesArgs& sa, const PrepArgs* pa) {
    if (T_ == 0 || N == 0) return DLRM_OK;
    T_ <<= ix.vshift;  // virtual tables (row-parity halves) of a forward-launch build
    hipStream_t s = ctx_stream(ctx);
    const unsigned* err = ctx_error_word(ctx);
    const int gesz = gdtype == DLRM_F32 ? 4 : 2;
    const int tesz = tdtype == DLRM_F32 ? 4 : 2;
    const bool aligned = tabs_aligned16 && (uintptr_t)grad % 16 == 0 && (grad_ld * gesz) % 16 == 0 &&
                         (grad_offset * gesz) % 16 == 0 && (D * gesz) % 16 == 0 && (D * tesz) % 16 == 0 && D % 4 == 0;
    bool done = false;
    const int64_t slots = (int64_t)T_ * (N + 1);  // (item counts stay in int)
    if (aligned && slots < (1ll << 31)) {
        const int vpr = D * gesz / 16;
        by_dtypes<R>(tdtype, gdtype, [&](auto tt, auto gt) {
            done = dispatch_apply<decltype(tt), decltype(gt), R>(vpr, s, ix, tabs, T_, L, grad, grad_ld, grad_offset, rule, N,
                                                                 err, sa, pa);
        });
    }
    if (!done && pa) launch_step_index(s, *pa);
    if (!done) {
        const int64_t gx0 = (N * D + 255) / 256;
        const unsigned gx = (unsigned)(gx0 < 1 ? 1 : (gx0 > 4096 ? 4096 : gx0));
        const int64_t hx0 = ((N / (kChunk + 1)) * D + 255) / 256;
        const unsigned hx = (unsigned)(hx0 < 1 ? 1 : (hx0 > 1024 ? 1024 : hx0));
        by_dtypes<R>(tdtype, gdtype, [&](auto tt, auto gt) {
            typedef decltype(tt) TT;
            typedef decltype(gt) GT;
            hipLaunchKernelGGL((sgd_chunks_scalar<TT, GT, R>), dim3(gx, T_), dim3(256), 0, s, ix, tabs, D, L,
                               (const GT*)grad, grad_ld, grad_offset, rule, err);
            hipLaunchKernelGGL((sgd_hot_scalar<TT, GT, R>), dim3(hx, T_), dim3(256), 0, s, ix, tabs, D, L, (const GT*)grad,
                               grad_ld, grad_offset, rule, err);
            if (sa.single)
                hipLaunchKernelGGL((sgd_singles_scalar<TT, GT, R>), dim3(gx, T_ >> ix.vshift), dim3(256), 0, s, sa, ix.cap,
                                   tabs, D, L, (const GT*)grad, grad_ld, grad_offset, rule, err);
        });
    }
    return ctx_hip(ctx, hipGetLastError(), "sgd_apply launch");
}


}  // namespace dlrm
