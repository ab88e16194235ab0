// build_plan.hpp — which index build a batch takes: decided here, once, as a pure function.
//
// Host only: no HIP header, `g++ -std=c++17` compiles it alone (tests/test_build_plan_host.py).  It
// holds the size constants the choice rests on (common.hpp includes it: the kernels read the same
// values), the environment knobs as a plain struct, and plan_build(): from the entry point that asks
// (BuildSite), the indexer's shape, the positions per table, the knobs and the shape facts only the
// kernels' units know (BuildCaps), to the form that runs and everything the host records about it
// (BuildPlan).  abi.cpp's entry points are checks -> plan_build -> run_build -> record_build; the
// launchers take the form and hold no size threshold.  DESIGN.md §20 has the table.
#pragma once
#include <stdint.h>

#include "../../include/dlrm_hip.h"

#if defined(__HIPCC__)
#define DLRM_HD __host__ __device__
#else
#define DLRM_HD
#endif

namespace dlrm {

constexpr int kFastMaxN = 4096;     // in-LDS indexer (indexer.hpp): positions per table
constexpr int kHixMaxN = 1 << 20;   // hash indexer (hashindex.hip): positions per table
constexpr int kStepIndexMaxN = 2048;  // the forward-launch indexer (interact.hip): positions per table
constexpr int kArgTables = 32;  // table pointers that travel by value in a forward kernel's arguments (common.hpp TabPtrs)
// The optimizer rules of the update and of the training step (common.hpp BoundRule; interact_plan.hpp: the step
// backward's forms per rule)
// (the last two: the Adagrad rules with the stochastic store -- an update only, no step backward has them)
enum {
    kRuleDescent = 0, kRuleSplit, kRuleAdagrad, kRuleRowwise, kRuleStochastic, kRuleStochasticAdagrad,
    kRuleStochasticRowwise, kNumRules
};
// the wave build (indexer.hpp wave_build_group) of the next batch (in the apply launch) or of a
// prepared batch (dlrm_indexer_prepare), and the bag build's per-part sort: up to kWaveMaxN
// positions per table, as 16 parts per 2048 positions (2^wave_vshift(N) parts per table; a part
// averages <= 128 positions).  The in-apply build (dlrm_step_bwd_prepare) takes up to
// kWaveApplyMaxN (its scan build keeps a quarter of the table's indices in registers).
constexpr int kWaveMaxN = 32768;
constexpr int kWaveApplyMaxN = 16384;
constexpr int kWaveMaxVshift = 8;
DLRM_HD constexpr int wave_vshift(int64_t N) {
    return N <= 2048 ? 4 : (N <= 4096 ? 5 : (N <= 8192 ? 6 : (N <= 16384 ? 7 : 8)));
}
// the next batch's split build in the apply launch (indexer.hpp wave_build_group): parts per
// table, one wave each, 4 per workgroup (>= 4)
#ifndef DLRM_WAVE_PARTS
#define DLRM_WAVE_PARTS 16
#endif
constexpr int kWaveBuildParts = DLRM_WAVE_PARTS;
constexpr int kWaveGroupParts = 4;  // parts (waves) of one build workgroup (indexer.hpp kWaveParts)
// split builds of kFastMaxN < N <= kPartsMaxN positions per table: the in-LDS build (1024
// threads x 8 positions) over 2^kPartsLog2 parts per table (by the row's low bits), each part's
// workgroup sized for the worst case (all N positions in one part)
constexpr int kPartsMaxN = 8192;
#ifndef DLRM_BUILD_PARTS_LOG2
#define DLRM_BUILD_PARTS_LOG2 2
#endif
constexpr int kPartsLog2 = DLRM_BUILD_PARTS_LOG2;
#ifndef DLRM_STEP_PARTS_DEFAULT
#define DLRM_STEP_PARTS_DEFAULT 4
#endif
constexpr int kStepParts = DLRM_STEP_PARTS_DEFAULT;

// Comparison knobs: every environment variable the library reads, read once (abi.cpp knobs()), in
// this one place.  0 = the default (the measured-best form); a non-zero value forces a variant for
// A/B runs.  None is needed for correctness.  plan_build takes them as an argument.
struct Knobs {
    int step_parts;   // DLRM_STEP_PARTS (4/8/16/32; below 4: 4): parts per table of the wave builds of <= 2048
                      // positions (the forward's launch, the apply's launch, dlrm_indexer_prepare); set, it
                      // also overrides dlrm_indexer_set_parts
    int build_parts;  // DLRM_BUILD_PARTS (2/4/8): parts of the in-LDS parts build, 4096 < N <= 8192
    int relu_1pass;   // DLRM_RELU_2PASS=0: the one-launch (last-arriver) relu seam instead of two launches
    int bwd_ys_body;  // DLRM_BWD_YS=0: the bwd_body kernel for a materialized ys with 33..96 features
    int bwd_nosplit;  // DLRM_BWD_SPLIT=0: the one-wave step backward instead of the split kernel
    int bwd_spb;      // DLRM_BWD_SPB (2/4/8): samples per block of the split step backward
    int bwd_cpl;      // DLRM_BWD_CPL (4/8): columns per lane of the bf16 split step backward
    int upd_sbu;      // DLRM_UPD_SBU (1/2): super-blocks in flight in the one-wave step backward
    int wave_rounds;  // DLRM_WAVE_ROUNDS=1: the wave build in rounds above 2048 positions per table
                      // instead of the scan build
    int bag_hash;     // DLRM_BAG_WAVE=0: dlrm_indexer_build of 8192 < N <= 32768 positions per table (pooled
                      // bags) by the hash build instead of the bag build
    int bag_vs;       // DLRM_BAG_VS (2..wave_vshift(capacity)): log2 parts per table of dlrm_indexer_build's bag
                      // build (default wave_vshift(N) - 1; dlrm_indexer_build_split's does not read it)
    int bag_split;    // DLRM_BAG_SPLIT=0: dlrm_indexer_build_split of 4096 < N <= 32768 by the in-LDS parts /
                      // hash builds instead of the bag build
};

// Which entry point asks.
enum class BuildSite {
    Build,       // dlrm_indexer_build; every update without PREBUILT; the last resort of dlrm_step_fwd
    BuildSplit,  // dlrm_indexer_build_split
    Prepare,     // dlrm_indexer_prepare
    StepFwd,     // dlrm_step_fwd
    InApply,     // *_step_bwd_prepare: the next batch's build with the apply
    BwdGather,   // dlrm_interact_bwd_gather with an indexer
};

// What runs.
enum class BuildForm {
    None,        // nothing is built: BuildPlan::rc says whether that is a refusal
    Kept,        // StepFwd on a prepared indexer built from these indices: the gather alone, the build stands
    Lds2,        // in LDS, one workgroup per table, 2 positions per thread (N <= 2048)
    Lds4,        // ... 4 positions per thread (N <= 4096)
    LdsParts,    // in LDS over 2^vshift parts per table, 8 positions per thread (4096 < N <= 8192)
    Hash,        // hashindex.hip (N <= 2^20)
    Sorted,      // indexer_build_kernel<false>: one workgroup per table sorts in HBM, unsplit, any N
    Bag,         // count, place by part, per-part wave sort (4096 < N <= 32768)
    Wave,        // the wave build as its own launch, or as workgroups of an apply launch (InApply)
    InForward,   // in dlrm_step_fwd's launch: the wave build (vshift >= 2), else in LDS per table
    InBackward,  // in dlrm_interact_bwd_gather's launch (or, its shape's decision, the unsplit build before it)
};

// The wave build's kernel.  (The values are the apply launch's MODE - 2: apply_kernel.hpp.)
enum WaveKind { kWaveOneRound = 0, kWaveRounds = 1, kWaveScan = 3 };
// Which word takes the build's bounds errors: the ctx's flag, or one of the indexer's own two
// (dlrm_indexer::prep_err) where the build may run beside kernels that read the ctx's flag to
// decide their writes.
enum class ErrWord { Ctx, Prep0, Prep1 };

// The indexer as dlrm_indexer_create carved it (carve_* below) and dlrm_indexer_set_parts set it
struct IndexerShape {
    int64_t cap;     // positions per table it was created for
    int T, TV;       // tables; tables of the per-part arrays (8 T: the in-LDS parts build's layout)
    int64_t hsize;   // hash slots per table, 0: no hash arrays
    int parts_log2;  // dlrm_indexer_set_parts (0: the default)
};

// What only the kernels' units know of the call's shape, asked before plan_build, and the call's own flags
struct BuildCaps {
    bool prepared;    // StepFwd: the indexer holds a prepared build of these very indices, not yet consumed
    bool step_fwd;    // StepFwd: step_fwd_supported (interact.hip): launch_step_fwd has a kernel
    bool step_split;  // StepFwd: step_split_supported: the shape's backward takes a split indexer
    bool split_bwd;   // InApply: the rule's split backward exists (abi.cpp has_split_bwd; it implies 16-B aligned
                      // tables and <= 32 features)
    bool bwd_only;    // InApply: DLRM_STEP_BWD_ONLY (no apply launch to carry a build)
    bool idx_vec32;   // Prepare / InApply: int32 indices, every table's 16-B aligned (the scan build's loads)
    int cus;          // Prepare: compute units (the scan build's waves per workgroup)
};

struct BuildPlan {
    BuildForm form = BuildForm::None;
    int rc = DLRM_OK;   // None: DLRM_E_UNSUPPORTED = the entry point refuses (its message: abi.cpp refuse_build)
    int vshift = 0;     // IndexerDev::vshift of the build
    bool split = false;     // once-hit positions flagged, not listed
    bool has_map = false;   // IndexerDev::has_map: flat item map, a table's parts packed
    ErrWord err = ErrWord::Ctx;
    bool build_err = false;  // IndexerDev::build_err = that word: the apply of this indexer folds it into the ctx's
    bool side = false;       // on the ctx's side stream, beside the fused forward
    bool prepared = false;   // the next dlrm_step_fwd of these indices only gathers
    int kind = kWaveOneRound;  // Wave (and InForward with vshift >= 2: one round)
    int waves = 0;             // Prepare: waves per workgroup (0: not the host's decision)
};

// ---- what dlrm_indexer_create carves, from the same thresholds
// virtual tables per table: 8 for the in-LDS parts build (v * cap slots per part; vshift <= 3) of an indexer
// whose capacity is in its range, else one: every wave build packs its parts per table
constexpr int carve_virtual_tables(int64_t cap) { return cap > kFastMaxN && cap <= kPartsMaxN ? 8 : 1; }
// the hash arrays exist when a build can exceed the in-LDS indexer
constexpr bool carve_hash(int64_t cap) { return cap > kFastMaxN; }

// Whether a wave build of N positions per table fits this indexer (compact layout: any parts; the flat
// records hold global perm entries in int32).
inline bool wave_fits(const IndexerShape& s, int64_t N) {
    return N <= s.cap && N <= kWaveMaxN && (int64_t)(s.T > 0 ? s.T : 1) * s.cap < (1ll << 31);
}

// log2 of a parts knob, rounded down, at most 32 parts
inline int parts_knob_log2(int p) { return p >= 32 ? 5 : (p >= 16 ? 4 : (p >= 8 ? 3 : (p >= 4 ? 2 : (p >= 2 ? 1 : 0)))); }

// vshift of the wave build of N positions per table: up to 2048 positions the indexer's set_parts unless
// DLRM_STEP_PARTS is set, then that knob, then 16 parts, never fewer than 4; above, 16 parts per 2048 positions
inline int wave_parts_log2(const IndexerShape& s, int64_t N, const Knobs& k) {
    if (N > kStepIndexMaxN) return wave_vshift(N);
    if (s.parts_log2 && !k.step_parts) return s.parts_log2;
    const int vs = parts_knob_log2(k.step_parts > 0 ? k.step_parts : kWaveBuildParts);
    return vs < 2 ? 2 : vs;
}

// int32 indices, every table's 16-B aligned: the scan build's vector loads (BuildCaps::idx_vec32)
inline bool idx_vec32(const void* idx, int itype, int64_t tstride) {
    return itype == DLRM_I32 && (uintptr_t)idx % 16 == 0 && (tstride * 4) % 16 == 0;
}
// The wave build's kernel for N positions per table.
// The one copy: plan_build, launch_step_index (update.hip) and the apply launch that carries a build
// (apply_kernel.hpp) ask it.
inline int wave_kind(int64_t N, bool vec32, const Knobs& k) {
    if (N <= kStepIndexMaxN) return kWaveOneRound;
    return !k.wave_rounds && vec32 && N % 4 == 0 ? kWaveScan : kWaveRounds;
}
// Waves per workgroup of the wave build's own launch: the scan build takes 16 when every workgroup is
// resident at once (one per CU), else 8 (two per CU) -- a second round of workgroups would double the
// build -- and always 16 above kWaveApplyMaxN, where 16 waves keep 8 pieces each in registers
inline int wave_waves(int kind, int64_t N, int64_t groups, int cus) {
    if (kind != kWaveScan) return kWaveGroupParts;
    return N > kWaveApplyMaxN || groups <= cus ? 16 : 8;
}

// The build with a launch of its own (update.hip launch_indexer_build) for N positions per table:
// vshift > 0 is the in-LDS parts build (the caller found has_parts).  None: a split build above the hash build.
inline BuildForm standalone_form(int64_t N, int64_t hsize, bool split, int vshift = 0) {
    if (vshift > 0) return BuildForm::LdsParts;
    if (N <= kStepIndexMaxN) return BuildForm::Lds2;
    if (N <= kFastMaxN) return BuildForm::Lds4;  // (8 positions per thread, one workgroup per table: slower than
                                                 // the hash build at N = 8192; in 4 parts per table the faster one)
    if (hsize && N <= kHixMaxN) return BuildForm::Hash;
    return split ? BuildForm::None : BuildForm::Sorted;
}

// vshift of the in-LDS parts build where a split build of N positions takes it (the indexer carved for it), else 0
inline int lds_parts_vshift(const IndexerShape& s, int64_t N, bool split, const Knobs& k) {
    const int p = k.build_parts ? k.build_parts : (1 << kPartsLog2);
    const int lg = p >= 8 ? 3 : (p >= 4 ? 2 : 1);
    const bool has_parts = (int64_t)s.TV >= ((int64_t)s.T << lg) && s.T > 0;
    return split && N > kFastMaxN && N <= kPartsMaxN && has_parts ? lg : 0;
}

// dlrm_indexer_build (force_split = false) and dlrm_indexer_build_split: a launch of its own on the ctx's stream.
// OPEN: both raise bounds errors on the ctx's flag although a caller may run them on a side stream
// beside a step whose kernels read that flag to decide their writes.  The fix is err = ErrWord::Prep0 (cleared
// before the launch, as Prepare's) and build_err = true on these two rows; it changes behaviour, so it is the next
// change's, with ADVICE's tests.
inline BuildPlan plan_standalone(bool force_split, const IndexerShape& s, int64_t N, const Knobs& k) {
    BuildPlan p;
    // the split form where the builds support it: once-hit positions flagged (single[]) instead of listed as
    // one-position chunks; the apply then updates them with no descriptor read
    p.split = force_split || N <= kFastMaxN || (s.hsize && N <= kHixMaxN);
    // the bag build above the in-LDS builds (pooled bags, the next batch of B = 8192 beside its step): half the
    // parts of the wave builds (128 to 256 positions per part)
    const bool bag = force_split ? k.bag_split && N > kFastMaxN && wave_fits(s, N)
                                 : p.split && N > kPartsMaxN && wave_fits(s, N) && !k.bag_hash;
    if (bag) {
        p.form = BuildForm::Bag;
        const bool forced = !force_split && k.bag_vs >= 2 && k.bag_vs <= wave_vshift(s.cap < kWaveMaxN ? s.cap : kWaveMaxN);
        p.vshift = forced ? k.bag_vs : wave_vshift(N) - 1;
        p.has_map = true;
        return p;
    }
    p.vshift = lds_parts_vshift(s, N, p.split, k);
    p.form = standalone_form(N, s.hsize, p.split, p.vshift);
    if (p.form == BuildForm::None) p.rc = DLRM_E_UNSUPPORTED;
    return p;
}

inline BuildPlan plan_build(BuildSite site, const IndexerShape& s, int64_t N, const Knobs& k, const BuildCaps& c) {
    BuildPlan p;
    switch (site) {
    case BuildSite::Build: return plan_standalone(false, s, N, k);
    case BuildSite::BuildSplit: return plan_standalone(true, s, N, k);
    case BuildSite::Prepare:
    case BuildSite::InApply: {
        // InApply: the split backward's shapes only (the apply launch that carries the build has no once-hit
        // items); otherwise the plain step, and the next forward builds
        const bool ok = site == BuildSite::Prepare
                            ? wave_fits(s, N)
                            : N > 0 && s.T > 0 && N <= kWaveApplyMaxN && (s.T + 1 + 15) / 16 <= 2 && wave_fits(s, N) &&
                                  c.split_bwd && !c.bwd_only;
        if (!ok) {
            p.rc = site == BuildSite::Prepare ? DLRM_E_UNSUPPORTED : DLRM_OK;
            return p;
        }
        p.form = BuildForm::Wave;
        p.vshift = wave_parts_log2(s, N, k);  // (never below 2)
        p.split = p.has_map = p.prepared = true;
        p.kind = wave_kind(N, c.idx_vec32, k);
        if (site == BuildSite::Prepare) {
            // its own word, not the ctx's flag: this build usually runs on a side stream beside the current step
            p.err = ErrWord::Prep0;
            p.build_err = true;
            p.waves = wave_waves(p.kind, N, ((int64_t)s.T << p.vshift) / kWaveGroupParts, c.cus);
        } else {
            p.err = ErrWord::Prep1;  // (nothing reads it: the forward of the same indices raises the errors)
        }
        return p;
    }
    case BuildSite::StepFwd: {
        if (c.prepared) {  // (what record_build wrote for that build stands: nothing else of the plan is read)
            p.form = BuildForm::Kept;
            return p;
        }
        p.split = true;
        if (c.step_fwd) {  // the build in the forward's launch: the wave build (it also writes the apply's item map)
            p.form = BuildForm::InForward;
            p.vshift = s.cap <= kWaveApplyMaxN && wave_fits(s, N) ? wave_parts_log2(s, kStepIndexMaxN, k) : 0;
            p.has_map = p.vshift >= 2;
            return p;
        }
        if (c.step_split && N <= kFastMaxN) {  // the fused forward, then the split build in LDS
            p.form = standalone_form(N, s.hsize, true);
            return p;
        }
        if (c.step_split && N <= kHixMaxN) {
            // large batch: the split build (once-hit rows left to dlrm_step_bwd) -- in LDS by table parts up to
            // kPartsMaxN, else the hash build -- on the side stream beside the fused forward
            p.vshift = lds_parts_vshift(s, N, true, k);
            if (p.vshift > 0 || s.hsize) {
                p.form = standalone_form(N, s.hsize, true, p.vshift);
                p.side = true;
                return p;
            }
        }
        return plan_standalone(false, s, N, k);  // the fused forward, then dlrm_indexer_build's row
    }
    case BuildSite::BwdGather:
        p.form = BuildForm::InBackward;
        return p;
    }
    return p;
}

}  // namespace dlrm
