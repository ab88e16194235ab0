// bags_plan.hpp — the pooled lookup + interaction forward on fp32 / bf16 tables (bags.hip): its domain, its column
// block and its LDS, as pure functions.
//
// Host only, as q4_plan.hpp: no HIP header, `g++ -std=c++17` compiles it alone (tests/test_bags_plan_host.py).
// bags.hip's launcher asks these and nothing else; DESIGN.md section 32 restates them.
#pragma once
#include <stdint.h>

#include "../../include/dlrm_hip.h"

namespace dlrm {

constexpr int kBagTables = 95;  // F = T + 1 <= 96 features: NB = 1 .. 6, the range of dlrm_interact_fwd's MFMA kernel

inline bool bags_at(const void* p, int bytes) { return (uintptr_t)p % (unsigned)bytes == 0; }
inline int bags_esz(int dtype) { return dtype == DLRM_F32 ? 4 : 2; }
inline int bags_nb(int T) { return (T + 1 + 15) / 16; }

// dlrm_bags_interact_fwd has a kernel exactly here (else DLRM_E_UNSUPPORTED, nothing launched):
//  - lookups >= 1 (bags of any size, one-hot included) of 1 .. 95 tables;
//  - d a whole number of 16-B vectors (vec = 4 fp32 or 8 bf16 elements) and every table row 16-B aligned;
//  - x 16-B aligned with x_ld % vec == 0; ys none, or 16-B aligned with ys_ld % vec == 0 (with d % vec == 0 every
//    pooled row of it is then one run of 16-B stores).
// out takes any alignment and leading dimension.
inline bool bags_fused(int dtype, int d, int T, int lookups, bool tabs_aligned16, const void* x, int64_t x_ld,
                       const void* ys, int64_t ys_ld) {
    const int vec = dtype == DLRM_F32 ? 4 : 8;
    return lookups >= 1 && T >= 1 && T <= kBagTables && d > 0 && d % vec == 0 && tabs_aligned16 && bags_at(x, 16) &&
           x_ld % vec == 0 && (!ys || (bags_at(ys, 16) && ys_ld % vec == 0));
}

// The bytes of a row per column block: 512 where NB <= 3, else 256 (the two tiles of bags_lds_bytes stay within
// 64 KB), capped at the row rounded up to a column step (64 B: 16 fp32 or 32 bf16 columns).  A row of several blocks
// has 8 or 4 steps per block, an even number: a step's parity within its block is its parity within the row.
inline int bags_cb_bytes(int dtype, int d, int T) {
    const int64_t row = ((int64_t)d * bags_esz(dtype) + 63) / 64 * 64;
    const int cb = bags_nb(T) <= 3 ? 512 : 256;
    return row < cb ? (int)row : cb;
}

// Two operand tiles rows[16 NB][cb_bytes + 16]: the gather of unit u + 1 fills one while the Gram of unit u reads the
// other.  The row stride is an odd number of 16-B units (section 30's bank argument: the 16-B reads of 16 consecutive
// rows at one column fall in 16 distinct quarters of the 64 banks).  At most 2 * 48 * 528 = 50688 B (NB = 3) and
// 2 * 96 * 272 = 52224 B (NB = 6).
inline int bags_lds_bytes(int dtype, int d, int T) { return 2 * 16 * bags_nb(T) * (bags_cb_bytes(dtype, d, T) + 16); }

}  // namespace dlrm
