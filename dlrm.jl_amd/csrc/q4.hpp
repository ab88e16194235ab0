// q4.hpp — int4 row-quantized tables: the device descriptor and q4.hip's launchers (called by abi.cpp).
#pragma once
#include "common.hpp"
#include "q4_plan.hpp"

namespace dlrm {

// Device-side descriptor of one quantized table: rows r[nrows][S] of S = q4_row_bytes(D) bytes ({scale, bias}, then
// the codes); row0 = the rows of the tables before it (the quantizer and the dequantizer walk every table's rows as
// one range).
struct __attribute__((aligned(16))) Q4Desc {
    uint8_t* r;
    int64_t nrows;
    int64_t row0;
    int64_t pad_;
};

// src: the fp32 / bf16 tables' device descriptors (src16: every row 16-B aligned); dst / src: the quantized tables'
int launch_q4_quantize(dlrm_ctx* ctx, const TableDesc* src, int dtype, bool src16, const Q4Desc* dst, int T, int D,
                       int64_t rows);
int launch_q4_dequantize(dlrm_ctx* ctx, const Q4Desc* src, const TableDesc* dst, int dtype, bool dst16, int T, int D,
                         int64_t rows);
int launch_q4_maplookup(dlrm_ctx* ctx, const Q4Desc* tabs, int T, int D, const void* idx, int itype, int64_t tstride,
                        int base, int B, int L, int dtype, void* out, int64_t out_ld, int64_t out_off);
// htabs: the host copy of the descriptors (their pointers travel by value).  DLRM_E_UNSUPPORTED, nothing launched:
// q4_plan.hpp q4_fwd_fused says no.
int launch_q4_lookup_interact_fwd(dlrm_ctx* ctx, const Q4Desc* htabs, int T, int d, const void* idx, int itype,
                                  int64_t tstride, int base, int B, int L, int dtype, const void* x, int64_t x_ld,
                                  void* out, int64_t out_ld, int padding);
// tabs: the device descriptors.  DLRM_E_UNSUPPORTED, nothing launched: q4_plan.hpp q4_bags_fused says no.
int launch_q4_bags_interact_fwd(dlrm_ctx* ctx, const Q4Desc* tabs, int T, int d, const void* idx, int itype,
                                int64_t tstride, int base, int B, int L, int dtype, const void* x, int64_t x_ld,
                                void* out, int64_t out_ld, int padding);

}  // namespace dlrm
