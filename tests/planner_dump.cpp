// Prints the launch planners' records (nlspn_plan.h: res_plan, br_plan) as JSON for a fixed
// list of cases.  Host only: no device, no HIP header, no Python.  tests/test_planner_cpu.py
// compiles it, runs it and compares the output with tests/golden/resident_plans.json; it is
// also the program to run under -fsanitize=address,undefined.
//   g++ -std=c++17 -I nlspn_eccv20_amd/csrc tests/planner_dump.cpp -o planner_dump
#include <cstdio>
#include <string_view>

#include "nlspn_plan.h"

using namespace nlspn;

namespace {

struct FwdCase {
    const char *name;
    int cus, es, B, H, W, kh, kw, T;
    const char *sw;  // the A/B switch that differs from the default, or ""
};

// A call like nlspn_propagate's: every pointer given and aligned, raw offsets.
const FwdCase kFwd[] = {
    {"C1", 256, 4, 1, 228, 304, 3, 3, 18, ""},
    {"C2", 256, 4, 8, 228, 304, 3, 3, 18, ""},
    {"C3", 256, 4, 4, 240, 1216, 3, 3, 18, ""},
    {"C3 B=5", 256, 4, 5, 240, 1216, 3, 3, 18, ""},
    {"C5", 256, 2, 16, 228, 304, 1, 17, 36, ""},
    {"5x5", 256, 4, 2, 228, 304, 5, 5, 18, ""},
    {"smoke", 256, 4, 2, 48, 64, 3, 3, 18, ""},
    {"tiny", 256, 4, 1, 4, 4, 3, 3, 18, ""},
    {"W%4", 256, 4, 1, 13, 17, 3, 3, 18, ""},
    {"7x7", 256, 4, 2, 48, 64, 7, 7, 18, ""},
    {"T=1", 256, 4, 2, 48, 64, 3, 3, 1, ""},
    {"T=2", 256, 4, 2, 48, 64, 3, 3, 2, ""},
    {"C2 split=0", 256, 4, 8, 228, 304, 3, 3, 18, "NLSPN_RES_SPLIT=0"},
    {"C2 merge=0", 256, 4, 8, 228, 304, 3, 3, 18, "NLSPN_RES_MERGE=0"},
    {"C2 first=0", 256, 4, 8, 228, 304, 3, 3, 18, "NLSPN_RES_FIRST=0"},
    {"C1 split=0", 256, 4, 1, 228, 304, 3, 3, 18, "NLSPN_RES_SPLIT=0"},
    {"C3 merge=0", 256, 4, 4, 240, 1216, 3, 3, 18, "NLSPN_RES_MERGE=0"},
    {"C2 64 CUs", 64, 4, 8, 228, 304, 3, 3, 18, ""},
    {"C2 304 CUs", 304, 4, 8, 228, 304, 3, 3, 18, ""},
};

struct BwdCase {
    const char *name;
    int cus, B, H, W;
};
const BwdCase kBwd[] = {
    {"C2", 256, 8, 228, 304},
    {"C3", 256, 4, 240, 1216},
    {"smoke", 256, 2, 48, 64},
    {"tiny", 256, 1, 4, 4},
};

Switches switches_of(const char *sw) {
    const std::string_view s(sw);
    Switches w;
    if (s == "NLSPN_RES_SPLIT=0") w.res_split = 0;
    if (s == "NLSPN_RES_MERGE=0") w.res_merge = false;
    if (s == "NLSPN_RES_FIRST=0") w.res_first = false;
    return w;
}

void print_build(const char *key, const ResPlanRec &R, bool groups) {
    printf(", \"%s\": {\"NTC\": %d, \"GROUPS\": %s, \"FIRST\": %s, \"PXO\": %d}", key, groups ? R.ntc_merged : R.ntc,
           groups ? "true" : "false", R.first ? "true" : "false", R.split);
}

}  // namespace

int main() {
    printf("{\"forward\": [\n");
    for (size_t i = 0; i < sizeof(kFwd) / sizeof(kFwd[0]); ++i) {
        const FwdCase &c = kFwd[i];
        const Switches sw = switches_of(c.sw);
        ResPlanRec R{c.es, c.B, c.H, c.W, c.kh, c.kw, c.T, true, sw.res_first};
        const bool res = res_plan(c.cus, sw, R);
        // a merged plan: launch 0 runs the full groups, a partial last group has launch 1
        const int launches = R.merged ? (R.ngroups > R.nfull ? 2 : 1) : R.ngroups;
        printf("%s{\"name\": \"%s\", \"cus\": %d, \"dtype\": \"%s\", \"B\": %d, \"H\": %d, \"W\": %d, \"kh\": %d, "
               "\"kw\": %d, \"T\": %d, \"switch\": \"%s\", \"resident\": %s",
               i ? ",\n" : "", c.name, c.cus, c.es == 2 ? "f16" : "f32", c.B, c.H, c.W, c.kh, c.kw, c.T, c.sw,
               res ? "true" : "false");
        if (res) {
            printf(", \"Bg\": %d, \"gy\": %d, \"gx\": %d, \"nt\": %d, \"win_cells\": %d, \"split\": %d, \"first\": %s, "
                   "\"merged\": %s, \"groups\": %d, \"launches\": %d, \"grid\": [",
                   R.S.Bg, R.S.gy, R.S.gx, R.S.nt, R.S.win_cells, R.split, R.first ? "true" : "false",
                   R.merged ? "true" : "false", R.ngroups, launches);
            for (int k = 0; k < launches; ++k) printf("%s%u", k ? ", " : "", R.grid[R.merged && k == 1 ? R.ngroups - 1 : k]);
            printf("], \"lds_bytes\": %zu", R.lds);
            print_build("build", R, false);
            if (R.merged) print_build("build_merged", R, true);
        }
        printf("}");
    }
    printf("\n],\n\"backward\": [\n");
    for (size_t i = 0; i < sizeof(kBwd) / sizeof(kBwd[0]); ++i) {
        const BwdCase &c = kBwd[i];
        BrPlan P;
        const bool ok = br_plan(c.B, c.H, c.W, c.cus, P);
        printf("%s{\"name\": \"%s\", \"cus\": %d, \"B\": %d, \"H\": %d, \"W\": %d, \"ok\": %s, \"Bl\": %d, \"py\": %d, "
               "\"px\": %d, \"PR\": %d, \"PC\": %d}",
               i ? ",\n" : "", c.name, c.cus, c.B, c.H, c.W, ok ? "true" : "false", P.Bl, P.py, P.px, P.PR, P.PC);
    }
    printf("\n]}\n");
    return 0;
}
