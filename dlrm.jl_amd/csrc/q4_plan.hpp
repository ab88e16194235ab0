// q4_plan.hpp — which kernel a call on int4 row-quantized tables launches: decided here, once, as pure functions.
//
// Host only, as q8_plan.hpp: no HIP header, `g++ -std=c++17` compiles it alone (tests/test_q4_host.py).
// q4.hip's launchers ask these and nothing else; DESIGN.md section 29 restates them.
#pragma once
#include <stdint.h>

#include "../../include/dlrm_hip.h"

namespace dlrm {

constexpr int kQ4ArgTables = 31;  // tables whose pointers the fused forward takes by value (F = T + 1 <= 32: NB <= 2)

// A row: {scale, bias} (8 bytes), then two codes per byte, padded to a whole number of 8-byte pieces (16 codes).
inline int64_t q4_row_bytes(int D) { return 8 + 8 * (((int64_t)D + 15) / 16); }

inline bool q4_at(const void* p, int bytes) { return (uintptr_t)p % (unsigned)bytes == 0; }

// Every quantized row is 8-B aligned (dlrm_q4_tables_create refuses anything else), so a lane's 16 codes always
// leave and arrive as one 8-byte piece.  What varies is the other side: the quantizer, the dequantizer and the
// gather move 16 elements of it per lane in 16-B vectors where D % 16 == 0 and every row of it starts on a 16-B
// boundary (rows16: the fp32 / bf16 table set's rows, or the gather's output rows); anything else takes the
// element-wise kernels, with the same results.
inline bool q4_rows_vec(int D, bool rows16) { return D % 16 == 0 && rows16; }
inline bool q4_out_rows16(int dtype, const void* out, int64_t out_ld, int64_t out_offset) {
    const int esz = dtype == DLRM_F32 ? 4 : 2;
    return q4_at(out, 16) && (out_ld * esz) % 16 == 0 && (out_offset * esz) % 16 == 0;
}

// dlrm_q4_lookup_interact_fwd has a fused kernel exactly here (else DLRM_E_UNSUPPORTED, nothing launched):
//  - one-hot indices (lookups == 1) of 1 .. 31 tables (F = T + 1 <= 32 features: one or two 16-row MFMA blocks);
//  - d % 16 == 0: a row's codes are whole 8-byte pieces with no pad nibble, and a lane of the MFMA layout owns 4
//    (fp32) or 8 (bf16) consecutive codes that never straddle d;
//  - x 16-B aligned with x_ld a whole number of 16-B vectors (the interaction forward's own condition).
// The rows need nothing beyond their 8-B alignment; out takes any alignment and leading dimension.
inline bool q4_fwd_fused(int dtype, int d, int T, int lookups, const void* x, int64_t x_ld) {
    const int vec = dtype == DLRM_F32 ? 4 : 8;
    return lookups == 1 && T >= 1 && T <= kQ4ArgTables && d % 16 == 0 && q4_at(x, 16) && x_ld % vec == 0;
}

// dlrm_q4_bags_interact_fwd (q4_bags_fwd_kernel: a workgroup per sample pools the bags into an LDS operand tile and
// runs the Gram from it) has a kernel exactly here (else DLRM_E_UNSUPPORTED, nothing launched):
//  - lookups >= 1 (bags of any size, one-hot included) of 1 .. 95 tables (F = T + 1 <= 96 features: NB = 1 .. 6 MFMA
//    row blocks, the range in which dlrm_interact_fwd runs its MFMA kernel);
//  - d % 16 == 0 and x as for q4_fwd_fused.
constexpr int kQ4BagTables = 95;
inline bool q4_bags_fused(int dtype, int d, int T, int lookups, const void* x, int64_t x_ld) {
    const int vec = dtype == DLRM_F32 ? 4 : 8;
    return lookups >= 1 && T >= 1 && T <= kQ4BagTables && d % 16 == 0 && q4_at(x, 16) && x_ld % vec == 0;
}

// The operand tile rows[16 NB][CB + pad] of the element type.  CB, the column block: the whole d, rounded up to a
// column step (16 fp32 or 32 bf16 columns), where a row of it is at most 512 B (d <= 128 fp32, d <= 256 bf16), else 128
// columns at a time.  pad = 16 B: the row stride is an odd number of 16-B units, so the 16-B reads of 16 consecutive
// rows at one column fall in 16 distinct quarters of the 64 banks.  At most 96 * 528 = 50688 B (F = 96).
inline int q4_bags_cb(int dtype, int d) {
    const int esz = dtype == DLRM_F32 ? 4 : 2, cols = dtype == DLRM_F32 ? 16 : 32;
    return (int64_t)d * esz <= 512 ? (d + cols - 1) / cols * cols : 128;
}
inline int q4_bags_lds_bytes(int dtype, int d, int T) {
    const int esz = dtype == DLRM_F32 ? 4 : 2, NB = (T + 1 + 15) / 16;
    return 16 * NB * (q4_bags_cb(dtype, d) * esz + 16);
}

}  // namespace dlrm
