// Drives csrc/pm_plan.cpp's plan_trace with TraceShape::mark (pm_set_caustic_map)
// on the CPU for tests/test_caustic_map.py: trace_plan_check.cpp's command with
// the mark switch in front,
//
//   plan MARK PATHS MPC ALIGNED MODE WIDE DEPTH LDS POOL_STACK TRACE_POOL TRACE_HOLD CUS  CAP V(12)
//     -> plan FAMILY POOLED LSTK POOL_PATHS GRID LDS LDS_HOLD HOLD HOLD_LAUNCH SPILL_ENTRIES SPILL_STRIDE | F:H:BYTES ...
//
// and the same occupancy table in place of the device.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pm_plan.h"

using namespace pm;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd != "plan") {
            fprintf(stderr, "unknown command: %s\n", cmd.c_str());
            return 1;
        }
        TraceShape sh;
        int mark = 0, aligned = 0, pool = 0, hold = 0;
        long long paths = 0;
        size_t cap = 0;
        int regs[12];
        in >> mark >> paths >> sh.mpc >> aligned >> sh.mode >> sh.wide >> sh.stack_depth >> sh.lds_bytes >> sh.pool_stack >> pool >>
            hold >> sh.cus >> cap;
        for (int &v : regs) in >> v;
        if (!in) {
            fprintf(stderr, "bad plan command: %s\n", line.c_str());
            return 1;
        }
        sh.mark = mark != 0;
        sh.path_count = paths; sh.slots_aligned = aligned != 0; sh.trace_pool = pool != 0; sh.trace_hold = hold != 0;
        struct Asked { int family, hold; size_t lds; };
        std::vector<Asked> asked;
        const TracePlan pl = plan_trace(sh, [&](TraceFamily f, bool h, size_t lds) {
            asked.push_back({(int)f, h ? 1 : 0, lds});
            if (cap == 0) return 0;
            const int blocks_regs = regs[2 * (int)f + (h ? 1 : 0)] / (TRACE_BLOCK / 64);
            const size_t blocks_lds = lds ? cap / lds : (size_t)blocks_regs;
            return (int)std::min<size_t>(blocks_regs, blocks_lds) * (TRACE_BLOCK / 64);
        });
        printf("plan %d %d %d %lld %lld %zu %zu %d %d %d %u |", (int)pl.family, pl.pooled ? 1 : 0, pl.lstk, (long long)pl.pool_paths,
               (long long)pl.grid_blocks, pl.lds, pl.lds_hold, pl.hold, pl.hold_launch ? 1 : 0, pl.spill_entries, pl.spill_stride);
        for (const Asked &a : asked) printf(" %d:%d:%zu", a.family, a.hold, a.lds);
        printf("\n");
    }
    return 0;
}
