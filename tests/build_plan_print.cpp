// Prints plan_build's answer for every case on stdin (tests/test_build_plan_host.py; tools/launch_trace.py's rows
// are the same ones).  Host only: it includes build_plan.hpp and nothing else of the library.
//
// One case per line, 20 integers:
//   site cap T TV hsize parts_log2 N  step_parts build_parts bag_hash bag_vs bag_split wave_rounds
//   prepared step_fwd step_split split_bwd bwd_only idx_vec32 cus
// One answer per line:
//   form kind vshift split has_map err side rc prepared build_err carve_tv carve_hash
#include <cstdio>

#include "../dlrm.jl_amd/csrc/build_plan.hpp"

using namespace dlrm;

static const char* form_name(BuildForm f) {
    switch (f) {
    case BuildForm::None: return "none";
    case BuildForm::Kept: return "kept";
    case BuildForm::Lds2: return "lds2";
    case BuildForm::Lds4: return "lds4";
    case BuildForm::LdsParts: return "lds_parts";
    case BuildForm::Hash: return "hash";
    case BuildForm::Sorted: return "sorted";
    case BuildForm::Bag: return "bag";
    case BuildForm::Wave: return "wave";
    case BuildForm::InForward: return "in_forward";
    case BuildForm::InBackward: return "in_backward";
    }
    return "?";
}

int main() {
    long long v[20];
    for (;;) {
        for (int i = 0; i < 20; ++i)
            if (scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 2;
        const IndexerShape s{v[1], (int)v[2], (int)v[3], v[4], (int)v[5]};
        Knobs k{};
        k.step_parts = (int)v[7];
        k.build_parts = (int)v[8];
        k.bag_hash = (int)v[9];
        k.bag_vs = (int)v[10];
        k.bag_split = (int)v[11];
        k.wave_rounds = (int)v[12];
        const BuildCaps c{v[13] != 0, v[14] != 0, v[15] != 0, v[16] != 0, v[17] != 0, v[18] != 0, (int)v[19]};
        const BuildPlan p = plan_build((BuildSite)v[0], s, v[6], k, c);
        const bool wave = p.form == BuildForm::Wave || (p.form == BuildForm::InForward && p.vshift >= 2);
        char kind[16] = "-";
        if (wave)
            snprintf(kind, sizeof kind, "%s%.0d", p.kind == kWaveScan ? "scan" : (p.kind == kWaveRounds ? "rounds" : "one"),
                     p.kind == kWaveScan ? p.waves : 0);
        printf("%s %s %d %d %d %s %d %d %d %d %d %d\n", form_name(p.form), kind, p.vshift, (int)p.split, (int)p.has_map,
               p.err == ErrWord::Ctx ? "ctx" : (p.err == ErrWord::Prep0 ? "prep0" : "prep1"), (int)p.side, p.rc,
               (int)p.prepared, (int)p.build_err, carve_virtual_tables(s.cap) * s.T, (int)carve_hash(s.cap));
    }
}
