// Prints br_plan's partition (nlspn_plan.h) for one shape: "ok Bl py px PR PC".  Host only, as
// tests/planner_dump.cpp; tests/test_gpu_backward_elem.py uses it to say how far a failing
// element lies from the nearest part seam.
//   g++ -std=c++17 -I nlspn_eccv20_amd/csrc tests/br_plan_query.cpp -o br_plan_query
//   br_plan_query B H W CUS
#include <cstdio>
#include <cstdlib>

#include "nlspn_plan.h"

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    nlspn::BrPlan P;
    const bool ok = nlspn::br_plan(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), P);
    printf("%d %d %d %d %d %d\n", ok ? 1 : 0, P.Bl, P.py, P.px, P.PR, P.PC);
    return 0;
}
