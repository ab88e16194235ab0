// q8_plan.hpp — which kernel a call on int8 row-quantized tables launches: decided here, once, as pure functions.
//
// Host only, as interact_plan.hpp: no HIP header, `g++ -std=c++17` compiles it alone (tests/test_q8_host.py).
// q8.hip's launchers ask these and nothing else; DESIGN.md section 25 restates them.
#pragma once
#include <stdint.h>

#include "../../include/dlrm_hip.h"

namespace dlrm {

constexpr int kQ8ArgTables = 31;  // tables whose pointers the fused forward takes by value (F = T + 1 <= 32: NB <= 2)

// What the launchers read off pointers and leading dimensions: the one place that looks at an address.
inline bool q8_at(const void* p, int bytes) { return (uintptr_t)p % (unsigned)bytes == 0; }

// The quantizer, the dequantizer and the gather move 16 codes per lane where every code row starts on a 16-B
// boundary (q_align: the largest power of two <= 16 that divides every table's q pointer) and so does every row of
// the other side (rows16: the fp32 / bf16 table set's rows, or the gather's output rows).  Anything else takes the
// one-code-per-lane kernels, with the same results.
inline bool q8_rows_vec(int D, int q_align, bool rows16) { return D % 16 == 0 && q_align >= 16 && rows16; }
inline bool q8_out_rows16(int dtype, const void* out, int64_t out_ld, int64_t out_offset) {
    const int esz = dtype == DLRM_F32 ? 4 : 2;
    return q8_at(out, 16) && (out_ld * esz) % 16 == 0 && (out_offset * esz) % 16 == 0;
}

// dlrm_q8_lookup_interact_fwd has a fused kernel exactly here (else DLRM_E_UNSUPPORTED, nothing launched):
//  - one-hot indices (lookups == 1) of 1 .. 31 tables (F = T + 1 <= 32 features: one or two 16-row MFMA blocks);
//  - d a whole number of lane vectors: d % 4 == 0 for fp32 x / out, d % 8 == 0 for bf16 (a lane of the MFMA layout
//    reads 4 or 8 consecutive codes of a row per column step; columns of the last step past d read as zero);
//  - every code row aligned for that 4-B / 8-B load (q_align >= 4 / 8; d % 4 / 8 == 0 keeps the rows aligned);
//  - x 16-B aligned with x_ld a whole number of 16-B vectors (the interaction forward's own condition).
// out takes any alignment and leading dimension.
inline bool q8_fwd_fused(int dtype, int d, int T, int lookups, int q_align, const void* x, int64_t x_ld) {
    const int vec = dtype == DLRM_F32 ? 4 : 8;
    return lookups == 1 && T >= 1 && T <= kQ8ArgTables && d % vec == 0 && q_align >= vec && q8_at(x, 16) &&
           x_ld % vec == 0;
}

}  // namespace dlrm
