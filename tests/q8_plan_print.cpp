// Prints csrc/q8_plan.hpp's answers for the cases on stdin (tests/test_q8_host.py): one line per case,
//   dtype d T lookups q_align x_address x_ld rows16  ->  fused vec
// Its own main and only that header: compiling it with the host C++ compiler shows the header needs no HIP.
#include <cstdio>

#include "../dlrm.jl_amd/csrc/q8_plan.hpp"

int main() {
    int dtype, d, T, L, q_align, rows16;
    long long x_addr, x_ld;
    while (std::scanf("%d %d %d %d %d %lld %lld %d", &dtype, &d, &T, &L, &q_align, &x_addr, &x_ld, &rows16) == 8) {
        const bool fused = dlrm::q8_fwd_fused(dtype, d, T, L, q_align, (const void*)(uintptr_t)x_addr, (int64_t)x_ld);
        const bool vec = dlrm::q8_rows_vec(d, q_align, rows16 != 0);
        std::printf("%d %d\n", fused ? 1 : 0, vec ? 1 : 0);
    }
    return 0;
}
