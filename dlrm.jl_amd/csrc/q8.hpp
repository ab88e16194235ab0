// q8.hpp — int8 row-quantized tables: the device descriptor and q8.hip's launchers (called by abi.cpp).
#pragma once
#include "common.hpp"
#include "q8_plan.hpp"

namespace dlrm {

// Device-side descriptor of one quantized table: codes q[nrows][D], {scale, bias} sb[nrows]; row0 = the rows of the
// tables before it (the quantizer and the dequantizer walk every table's rows as one range).
struct __attribute__((aligned(16))) Q8Desc {
    uint8_t* q;
    float2* sb;
    int64_t nrows;
    int64_t row0;
};

// src: the fp32 / bf16 tables' device descriptors (src16: every row 16-B aligned); dst / src: the quantized tables'
int launch_q8_quantize(dlrm_ctx* ctx, const TableDesc* src, int dtype, bool src16, const Q8Desc* dst, int q_align, int T,
                       int D, int64_t rows);
int launch_q8_dequantize(dlrm_ctx* ctx, const Q8Desc* src, int q_align, const TableDesc* dst, int dtype, bool dst16,
                         int T, int D, int64_t rows);
int launch_q8_maplookup(dlrm_ctx* ctx, const Q8Desc* tabs, int q_align, int T, int D, const void* idx, int itype,
                        int64_t tstride, int base, int B, int L, int dtype, void* out, int64_t out_ld, int64_t out_off);
// htabs: the host copy of the descriptors (their pointers travel by value).  DLRM_E_UNSUPPORTED, nothing launched:
// q8_plan.hpp q8_fwd_fused says no.
int launch_q8_lookup_interact_fwd(dlrm_ctx* ctx, const Q8Desc* htabs, int q_align, int T, int d, const void* idx,
                                  int itype, int64_t tstride, int base, int B, int L, int dtype, const void* x,
                                  int64_t x_ld, void* out, int64_t out_ld, int padding);

}  // namespace dlrm
