// Prints csrc/bags_plan.hpp's answers (tests/test_bags_plan_host.py).  Per case on stdin,
//   dtype d T lookups tabs16 x_address x_ld ys_address ys_ld  ->  fused cb_bytes lds_bytes
// then "max" with the largest LDS over the whole domain (d up to 4096) and those at NB = 3 and NB = 6.
// Its own main and only that header: compiling it with the host C++ compiler shows the header needs no HIP.
#include <cstdio>

#include "../dlrm.jl_amd/csrc/bags_plan.hpp"

int main() {
    int dtype, d, T, L, tabs16, top[7] = {0, 0, 0, 0, 0, 0, 0};
    long long xa, x_ld, ya, ys_ld;
    while (std::scanf("%d %d %d %d %d %lld %lld %lld %lld", &dtype, &d, &T, &L, &tabs16, &xa, &x_ld, &ya, &ys_ld) == 9)
        std::printf("%d %d %d\n", (int)dlrm::bags_fused(dtype, d, T, L, tabs16 != 0, (const void*)(uintptr_t)xa, x_ld,
                                                        (const void*)(uintptr_t)ya, ys_ld),
                    dlrm::bags_cb_bytes(dtype, d, T), dlrm::bags_lds_bytes(dtype, d, T));
    for (int dt = 0; dt < 2; ++dt)
        for (T = 1; T <= dlrm::kBagTables; ++T)
            for (d = dt ? 8 : 4; d <= 4096; d += dt ? 8 : 4) {
                const int lds = dlrm::bags_lds_bytes(dt, d, T), nb = dlrm::bags_nb(T);
                top[0] = lds > top[0] ? lds : top[0];
                top[nb] = lds > top[nb] ? lds : top[nb];
            }
    std::printf("max %d %d %d\n", top[0], top[3], top[6]);
    return 0;
}
