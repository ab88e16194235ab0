// interact_plan.hpp — which interaction kernel a call launches: decided here, once, as a pure function.
//
// Host only, as build_plan.hpp: no HIP header, `g++ -std=c++17` compiles it alone (tests/test_interact_plan_host.py).
// interact.hip's launchers are interact_align -> plan_interact -> launch, and the *_supported queries that abi.cpp
// asks before it plans a build are the same plans' answers.  Grid and dynamic LDS are the launchers', beside the
// device types that size them.  DESIGN.md section 22 has the table of sites and forms.
#pragma once
#include "build_plan.hpp"

namespace dlrm {

constexpr int kBwdIndexMaxN = 2048;  // the backward-launch indexer (interact_bwd_index_kernel): positions per table

// Which launcher asks: launch_interact_fwd, launch_lookup_interact_fwd, launch_interact_bwd,
// launch_interact_bwd_gather without and with an indexer, launch_interact_bwd_blocked, launch_step_fwd, launch_step_bwd
enum class InteractSite { Fwd, LookupFwd, Bwd, BwdGather, BwdGatherIndexed, BwdBlocked, StepFwd, StepBwd };

struct InteractShape {
    int dtype, d, F, B, L;  // F: features (tables + 1)
    bool ys;                // LookupFwd keeps the gathered rows
};

// What the launchers read off pointers and leading dimensions.  The forward asks for 16-B fragment loads (vec = 4
// fp32 or 8 bf16 elements), the backward for 4-element ones: each site's condition is kept as it was.
struct InteractAlign {
    bool x_fwd, ys_fwd, d_fwd;  // x, ys (none: true) 16-B aligned with a leading dimension % vec == 0; d % vec == 0
    bool x_bwd, t_bwd, d_bwd;   // x, the materialized ys aligned to 4 elements, leading dimension % 4 == 0; d % 4 == 0
    bool dx, dt;                // dx, dt (the blocked backward's dst, ld 0) 16-B aligned, leading dimension % 4 == 0
    bool tabs_aligned16;
    bool tab_ptrs;  // fill_tab_ptrs would succeed: host descriptors, 1..kArgTables tables, each of < 2^32 - 1 rows
};
// The one place that looks at an address.  t: ys (forward) or the materialized ys (backward); max_rows: the largest
// table's rows, < 0 without host descriptors.
inline InteractAlign interact_align(int dtype, int d, const void* x, int64_t x_ld, const void* t, int64_t t_ld,
                                    const void* dx, int64_t dx_ld, const void* dt, int64_t dt_ld, bool tabs_aligned16,
                                    int T, int64_t max_rows) {
    const int vec = dtype == DLRM_F32 ? 4 : 8, esz = dtype == DLRM_F32 ? 4 : 2;
    const auto at = [](const void* p, int bytes) { return (uintptr_t)p % (unsigned)bytes == 0; };
    return InteractAlign{at(x, 16) && x_ld % vec == 0, at(t, 16) && t_ld % vec == 0, d % vec == 0,
                         at(x, 4 * esz) && x_ld % 4 == 0, at(t, 4 * esz) && t_ld % 4 == 0, d % 4 == 0,
                         at(dx, 16) && dx_ld % 4 == 0, at(dt, 16) && dt_ld % 4 == 0, tabs_aligned16,
                         max_rows >= 0 && T > 0 && T <= kArgTables && max_rows < (int64_t)UINT32_MAX};
}

enum class InteractKernel {
    None,       // nothing is launched: InteractPlan::rc says whether that is a refusal
    FwdScalar,  // interact_fwd_scalar<T>
    Fwd,        // interact_fwd_kernel<T, NB, fused, pooled, DC>
    FwdIndex,   // interact_fwd_index_kernel<T, NB, DC>
    BwdScalar,  // interact_bwd_scalar<T, gather>
    Bwd,        // interact_bwd_kernel<T, NB, gather>
    BwdIndex,   // interact_bwd_index_kernel<T, NB>
    BwdSplit,   // interact_bwd_split_kernel<T, NB, DC, SPB, WPS, mapped, CPL, ys, rule>
    BwdUpdate,  // interact_bwd_update_kernel<T, NB, SBU, DC, rule>
};

struct InteractPlan {
    InteractKernel kernel = InteractKernel::None;
    int rc = DLRM_OK;  // None: DLRM_E_UNSUPPORTED = the launcher refuses
    bool f32 = false;  // the element type T (the split rule's rows are bf16 whatever dtype says)
    int NB = 0, DC = 0, WPS = 0, CPL = 0, SPB = 0, SBU = 0;
    bool fused = false, pooled = false, gather = false, mapped = false, ys = false;
    bool tab_ptrs = false;     // the table pointers travel by value (TabPtrs filled)
    bool indexer = false;      // the index build rides in this launch
    bool build_first = false;  // BwdGatherIndexed with no such kernel: the indexer's own launch, then this one
};

// The forms <NB, WPS, CPL, SPB> of interact_bwd_split_kernel that exist for a rule (kRule*) and an element type.
// d = 128: two waves per sample (WPS 2, 4 samples per block),
// or 8 columns per lane (bf16 rows, one wave per sample, 2 samples per block); d <= 64: one wave per sample, 8
// samples per block.  Descent has them all, with 2, 4 or 8 samples per block at d = 128 (DLRM_BWD_SPB).  The other
// rules have the default samples per block only, and no form that would run below Descent's occupancy
// (DESIGN.md sections 14 and 15):
//  - 8 columns per lane with up to 16 features (NB = 1): the split write took that form from 6 to 5 waves per SIMD
//    (96 VGPRs against Descent's 80), so those shapes keep the two-wave form, which holds Descent's 8;
//  - with up to 16 features Descent's forms hold 8 waves per SIMD at 56..59 VGPRs, and the row-wise forms need
//    77..87, the element-wise one-wave form on fp32 tables 66.
// The split rule's rows live in bf16 tables, and so do the stochastic rule's: that rule has
// every default-geometry form of Descent on bf16 tables but the 8-column one with up to 16 features, as the split rule.
constexpr bool step_bwd_form(int rule, bool f32, int NB, int WPS, int CPL, int SPB) {
    const bool d128 = WPS == 2 || CPL == 8, descent = rule == kRuleDescent;
    if ((CPL == 8 && (f32 || WPS != 1)) || !(SPB == 2 || SPB == 4 || SPB == 8)) return false;
    if (SPB != (CPL == 8 ? 2 : (d128 ? 4 : 8))) return descent && d128;
    if (descent) return true;
    if (CPL == 8 && NB == 1) return false;
    if (rule == kRuleSplit || rule == kRuleStochastic) return !f32;
    // the seeded Adagrad rules (dlrm_sr_adagrad_step_bwd): their parents' forms on bf16 tables, but the two that the
    // Philox rounds at the write take below the parent -- the row-wise 8-column form (the
    // parent sits at the form's 168 VGPRs: 8 of them spilt) and the element-wise one-wave form with up to 16 features
    // (70 VGPRs against 63: 7 waves per SIMD against 8); those shapes keep the two-wave form or the gather backward
    if (rule == kRuleStochasticRowwise) return !f32 && CPL == 4 && step_bwd_form(kRuleRowwise, false, NB, WPS, CPL, SPB);
    if (rule == kRuleStochasticAdagrad)
        return !f32 && !(NB == 1 && WPS == 1) && step_bwd_form(kRuleAdagrad, false, NB, WPS, CPL, SPB);
    return rule == kRuleRowwise ? NB == 2 : !(NB == 1 && WPS == 1 && f32);
}

inline InteractPlan plan_interact(InteractSite site, const InteractShape& s, const InteractAlign& a, const Knobs& k,
                                  int rule = kRuleDescent) {
    typedef InteractKernel K;
    InteractPlan p;
    const int T = s.F - 1, NB = (s.F + 15) / 16, d = s.d;
    const bool fwd_x = a.x_fwd && a.d_fwd, fwd_ok = fwd_x && a.ys_fwd;  // the forward's condition: on x alone, with ys
    const bool gather_ok = a.d_bwd && a.tabs_aligned16 && a.x_bwd && a.dx && a.dt;  // the gather backward's
    const bool descent = rule == kRuleDescent, d_split = d == 128 || d <= 64;
    p.f32 = s.dtype == DLRM_F32;
    p.NB = NB;
    const auto refuse = [&] { return p = InteractPlan{K::None, DLRM_E_UNSUPPORTED}; };
    const auto run = [&](K kernel) { return p.kernel = kernel, p; };
    const auto split = [&](int DC, int SPB, int WPS, int CPL) {
        return p.DC = DC, p.SPB = SPB, p.WPS = WPS, p.CPL = CPL, run(K::BwdSplit);
    };
    // the one-wave-per-sample backward (NB = 8 would need > 64 KB of dynamic LDS), else the scalar kernel
    const auto bwd_body = [&](bool aligned) { return run(aligned && NB >= 1 && NB <= 7 ? K::Bwd : K::BwdScalar); };
    switch (site) {
    case InteractSite::Fwd:  // NB > 6 would exceed 256 VGPRs; odd alignments: the scalar kernel
        if (s.B == 0) return p;
        if (!(fwd_ok && NB >= 1 && NB <= 6)) return run(K::FwdScalar);
        p.DC = d == 128 ? 128 : 0;  // the BASELINE feature size, compiled for it
        return run(K::Fwd);
    case InteractSite::LookupFwd:
        if (s.B == 0) return p;
        if (T == 0 || !a.tabs_aligned16 || !fwd_ok || NB > 6) return refuse();
        // Pooled bags with ys kept: the many-wave pooled gather (maplookup) + the interaction on ys beat one wave
        // gathering T*L rows per sample (measured 489 vs 701 us at 64 x 256, L = 10); the caller's two-launch
        // fallback gives the same bits.
        if (s.L > 1 && s.ys && (int64_t)T * s.L > 64) return refuse();
        p.tab_ptrs = s.L == 1 && NB <= 2;
        if (p.tab_ptrs && !a.tab_ptrs) return refuse();  // (the two-launch form)
        p.fused = true;
        p.pooled = s.L > 1;
        p.DC = !p.pooled && d == 128 ? 128 : 0;
        return run(K::Fwd);
    case InteractSite::Bwd: {
        if (s.B == 0) return p;
        const bool aligned = a.d_bwd && a.t_bwd && a.dx && a.dt;
        // a materialized ys with 33..96 features (pooled bags): the split kernel's load plan, one wave per 64-column
        // super-block (the one-wave-per-sample bwd_body kernel spills at NB = 5 and ran the pooled backward at
        // 145 us); bit-identical (the same MFMA sums).  DLRM_BWD_YS = 0: bwd_body.
        const int wps = d >= 256 ? 4 : (d >= 128 ? 2 : 1);
        if (k.bwd_ys_body || !aligned || NB < 3 || NB > 6 || d != 64 * wps) return bwd_body(aligned);
        p.ys = true;
        return split(0, 1, wps, 4);
    }
    case InteractSite::BwdGather:
    case InteractSite::BwdGatherIndexed:
        p.gather = true;
        if (site == InteractSite::BwdGatherIndexed && s.B > 0 && T > 0) {
            p.indexer = gather_ok && NB <= 2 && (int64_t)s.B * s.L <= kBwdIndexMaxN;
            if (p.indexer) return run(K::BwdIndex);
            p.build_first = true;  // no fused form for this shape: the indexer's own launch, then the backward
        }
        return s.B == 0 ? p : bwd_body(gather_ok);
    case InteractSite::BwdBlocked:
        if (s.B == 0 || T == 0) return p;
        if (!gather_ok || NB > 7) return refuse();
        p.gather = p.mapped = true;
        // the step backward's kernel (two waves per sample at d = 128, one at d <= 64) with no once-hit update: every
        // table row's gradient goes to the send layout
        if (s.L == 1 && NB <= 2 && d_split && fwd_x) return d == 128 ? split(128, 4, 2, 4) : split(0, 2, 1, 4);
        return run(K::Bwd);
    case InteractSite::StepFwd:
        if (s.B == 0 || T == 0 || !a.tabs_aligned16 || !fwd_x || NB > 2 || s.B > kStepIndexMaxN || !a.tab_ptrs)
            return refuse();
        p.fused = p.tab_ptrs = p.indexer = true;
        p.DC = d == 128 ? 128 : 0;
        return run(K::FwdIndex);
    case InteractSite::StepBwd: {
        if (s.B == 0 || T == 0) return p;
        // the shapes whose backward takes a split indexer: F <= 32, 16-B aligned rows and x, whatever the batch size
        if (!a.tabs_aligned16 || !fwd_x || NB > 2) return refuse();
        // Descent and the split rule have every such shape (interact_bwd_update_kernel takes the d that
        // interact_bwd_split_kernel does not).  An Adagrad rule and the stochastic rule: d = 128 and d <= 64 only; any
        // other d and DLRM_BWD_SPLIT = 0 take the gather backward.  The row-wise rule also needs the vector apply's
        // summation order to exist for the shape (fp32 dt rows of d / 4 vectors, d / 4 a power of two: apply_kernel.hpp
        // dispatch_apply); the any-D kernels sum a row's squares in column order, which no lane layout here reproduces.
        const bool forms = !k.bwd_nosplit && d_split;
        if (!descent && rule != kRuleSplit && !forms) return refuse();
        const bool rowwise = rule == kRuleRowwise || rule == kRuleStochasticRowwise;
        if (rowwise && !(d >= 8 && (d & (d - 1)) == 0)) return refuse();
        p.f32 = p.f32 && rule != kRuleSplit;
        p.gather = true;
        if (!forms) {  // one super-block of T rows in flight: two (the gather backward's choice) spill here
            p.DC = descent && d == 128 ? 128 : 0;
            p.SBU = p.DC == 128 && k.upd_sbu == 2 ? 2 : 1;  // (DLRM_UPD_SBU)
            return run(K::BwdUpdate);
        }
        // bf16, B > 2048: 8 columns per lane, one wave per sample, 2 samples per block (kaggle-d128-b8192-bf16:
        // backward 52.2 -> 48.4 us, step 110.9 -> 103.3 us, r6q; at B = 2048 the two-wave form keeps the step shorter:
        // Terabyte rows 50.6 vs 48.7 M samples/s, r6s), where the rule has that form.  DLRM_BWD_CPL = 4 / 8 forces
        // either form and DLRM_BWD_SPB = 2, 4 or 8 the samples per block at d = 128: both are Descent's alone.
        const int cpl_env = descent ? k.bwd_cpl : 0, spb_in = descent && d == 128 ? k.bwd_spb : 0;
        const bool cpl8 =
            d == 128 && !p.f32 && (cpl_env ? cpl_env == 8 : s.B > 2048) && step_bwd_form(rule, p.f32, NB, 1, 8, 2);
        const int spb_env = spb_in >= 8 ? 8 : (spb_in >= 4 ? 4 : (spb_in > 0 ? 2 : 0)), wps = d == 128 && !cpl8 ? 2 : 1;
        const int spb = spb_env ? spb_env : (cpl8 ? 2 : (d == 128 ? 4 : 8));
        if (!step_bwd_form(rule, p.f32, NB, wps, cpl8 ? 8 : 4, spb)) return refuse();
        return split(d == 128 ? 128 : 0, spb, wps, cpl8 ? 8 : 4);
    }
    }
    return p;
}

}  // namespace dlrm
