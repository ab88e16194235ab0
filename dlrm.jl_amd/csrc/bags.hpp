// bags.hpp — the pooled lookup + interaction forward on fp32 / bf16 tables: bags.hip's launcher (called by abi.cpp).
#pragma once
#include "bags_plan.hpp"
#include "common.hpp"

namespace dlrm {

// tabs: the device descriptors.  ys may be null.  DLRM_E_UNSUPPORTED, nothing launched: bags_plan.hpp bags_fused says no.
int launch_bags_interact_fwd(dlrm_ctx* ctx, const TableDesc* tabs, bool tabs_aligned16, int T, int dtype, const void* idx,
                             int itype, int64_t tstride, int base, int L, int d, int B, const void* x, int64_t x_ld,
                             void* ys, int64_t ys_ld, void* out, int64_t out_ld, int padding);

}  // namespace dlrm
