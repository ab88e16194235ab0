// Prints csrc/q4_plan.hpp's answers for the cases on stdin (tests/test_q4_host.py): one line per case,
//   dtype d T lookups x_address x_ld rows16  ->  fused vec row_bytes
// Its own main and only that header: compiling it with the host C++ compiler shows the header needs no HIP.
#include <cstdio>

#include "../dlrm.jl_amd/csrc/q4_plan.hpp"

int main() {
    int dtype, d, T, L, rows16;
    long long x_addr, x_ld;
    while (std::scanf("%d %d %d %d %lld %lld %d", &dtype, &d, &T, &L, &x_addr, &x_ld, &rows16) == 7) {
        const bool fused = dlrm::q4_fwd_fused(dtype, d, T, L, (const void*)(uintptr_t)x_addr, (int64_t)x_ld);
        std::printf("%d %d %lld\n", fused ? 1 : 0, dlrm::q4_rows_vec(d, rows16 != 0) ? 1 : 0,
                    (long long)dlrm::q4_row_bytes(d));
    }
    return 0;
}
