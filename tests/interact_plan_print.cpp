// Prints plan_interact's answer for every case on stdin (tests/test_interact_plan_host.py; tools/launch_trace.py's
// rows are the same ones).  Host only: it includes interact_plan.hpp and nothing else of the library.
//
// One case per line, 23 integers (the addresses are never dereferenced: interact_align looks at their low bits):
//   site dtype d F B L ys  x x_ld t t_ld dx dx_ld dt dt_ld  tabs_aligned16 max_rows
//   bwd_ys_body bwd_nosplit bwd_spb bwd_cpl upd_sbu  rule
// One answer per line:
//   kernel rc f32 NB DC WPS CPL SPB SBU fused pooled gather mapped ys tab_ptrs indexer build_first
#include <cstdio>

#include "../dlrm.jl_amd/csrc/interact_plan.hpp"

using namespace dlrm;

static const char* kernel_name(InteractKernel k) {
    switch (k) {
    case InteractKernel::None: return "none";
    case InteractKernel::FwdScalar: return "fwd_scalar";
    case InteractKernel::Fwd: return "fwd";
    case InteractKernel::FwdIndex: return "fwd_index";
    case InteractKernel::BwdScalar: return "bwd_scalar";
    case InteractKernel::Bwd: return "bwd";
    case InteractKernel::BwdIndex: return "bwd_index";
    case InteractKernel::BwdSplit: return "bwd_split";
    case InteractKernel::BwdUpdate: return "bwd_update";
    }
    return "?";
}

int main() {
    long long v[23];
    for (;;) {
        for (int i = 0; i < 23; ++i)
            if (scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 2;
        const InteractShape s{(int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], v[6] != 0};
        const InteractAlign a = interact_align(s.dtype, s.d, (const void*)(uintptr_t)v[7], v[8], (const void*)(uintptr_t)v[9],
                                               v[10], (const void*)(uintptr_t)v[11], v[12], (const void*)(uintptr_t)v[13],
                                               v[14], v[15] != 0, s.F - 1, v[16]);
        Knobs k{};
        k.bwd_ys_body = (int)v[17];
        k.bwd_nosplit = (int)v[18];
        k.bwd_spb = (int)v[19];
        k.bwd_cpl = (int)v[20];
        k.upd_sbu = (int)v[21];
        const InteractPlan p = plan_interact((InteractSite)v[0], s, a, k, (int)v[22]);
        printf("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", kernel_name(p.kernel), p.rc, (int)p.f32, p.NB, p.DC,
               p.WPS, p.CPL, p.SPB, p.SBU, (int)p.fused, (int)p.pooled, (int)p.gather, (int)p.mapped, (int)p.ys,
               (int)p.tab_ptrs, (int)p.indexer, (int)p.build_first);
    }
}
