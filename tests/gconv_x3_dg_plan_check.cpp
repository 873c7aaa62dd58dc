// Host-only check of the tiling contract of the split-bf16 data-gradient presets
// (NLSPN_GCX3_DG_CONFIGS, csrc/nlspn_gconv_plan.h): tests/gconv_x3_plan_check.cpp's cell-by-cell
// staging and fragment check, that very code, run over the data-gradient list instead of the
// forward one (the kernel body, its staging and its fragment reads are shared; only the epilogue
// differs).  Same output and arguments; in addition
//     tile <preset> <gh> <gw>
// prints what gc_tile (the launcher's function) plans for that grid as one JSON object, the edge
// claims of tests/_gconv_x3_dgrad_cases.py being statements about it.
// tests/test_gconv_x3_dgrad_cpu.py builds and runs it.
#include "nlspn_gconv_plan.h"

#undef NLSPN_GCX3_CONFIGS
#define NLSPN_GCX3_CONFIGS(X) NLSPN_GCX3_DG_CONFIGS(X)
#define main plan_check_main
#include "gconv_x3_plan_check.cpp"
#undef main

#include <cstring>

int main(int argc, char **argv) {
    if (argc != 5 || std::strcmp(argv[1], "tile") != 0) return plan_check_main(argc, argv);
    std::vector<Preset> presets;
    NLSPN_GCX3_CONFIGS(NLSPN_GCX3_ROW)
    const int gh = std::atoi(argv[3]), gw = std::atoi(argv[4]);
    for (const Preset &p : presets) {
        if (p.id != std::atoi(argv[2])) continue;
        GcTiling t;
        const bool ok = gc_tile(p.g, gh, gw, t);
        const int bwl = gw - (t.nbands - 1) * t.bw;
        const GcWindow last = gc_window(p.g.mode, t.gh, t.gw, t.bw, t.npx, t.nbands - 1, t.tpb - 1);
        std::printf("{\"ok\": %d, \"nbands\": %d, \"bw\": %d, \"bwl\": %d, \"npx\": %d, \"npx_full\": %d, \"tpb\": %d, "
                    "\"bwmax\": %d, \"empty_last\": %d, \"wgco\": %d}\n",
                    ok ? 1 : 0, t.nbands, t.bw, bwl, t.npx, p.g.npx, t.tpb, gc_bwmax(p.g.mode, p.g.xp), last.empty ? 1 : 0,
                    p.g.wgco);
        return 0;
    }
    return 2;
}
