// Drives csrc/pm_plan.cpp on the CPU for tests/test_pass_plan.py: reads one
// command per line from stdin, answers each with one line on stdout. Floats
// cross as their bit patterns (hex), so nothing is rounded by printing.
//
//   grid LO(3) HI(3) ESTIMATOR SPAN R2      -> grid DX DY DZ NCELLS INV_CS
//   quant Q INIT H(64)                      -> quant BIN R2
//   bands N UNIT WORLD                      -> bands B:C,B:C|B:C,...   (one group per device)
// the R2Plan events (one plan per process run, `new Q` starts over); every
// answer ends with the plan's state, `| wanted accum dirty pending valid accum_init hist_init design_r2`:
//   new Q | active EST | landed INIT H(64) | due | issued STREAM | began FRESH
//   radius INIT FRESH | bin INIT STREAM | binned INIT | invalidate
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "pm_plan.h"

using namespace pm;

static float f_of(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static uint32_t u_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float read_f(std::istream &in) { uint32_t u = 0; in >> std::hex >> u >> std::dec; return f_of(u); }
static const void *stream_of(std::istream &in) { static const char ids[8] = {0}; int k = 0; in >> k; return k ? &ids[k & 7] : nullptr; }

static void state(const R2Plan &r) {
    printf(" | %d %d %d %d %d %08x %08x %08x\n", r.wanted, r.accum, r.dirty, r.pending, r.valid, u_of(r.accum_init),
           u_of(r.hist_init), u_of(r.design_r2));
}

int main() {
    R2Plan r;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "grid") {
            float lo[3], hi[3];
            for (float &v : lo) v = read_f(in);
            for (float &v : hi) v = read_f(in);
            int est = 0, span = 0;
            in >> est >> span;
            const GridDesc g = make_grid(lo, hi, est, span, read_f(in));
            if (u_of(g.gx) != u_of(lo[0]) || u_of(g.gy) != u_of(lo[1]) || u_of(g.gz) != u_of(lo[2])) return 2;
            printf("grid %d %d %d %u %08x\n", g.dx, g.dy, g.dz, g.ncells, u_of(g.inv_cs));
        } else if (cmd == "quant" || cmd == "landed") {
            double q = 0;
            if (cmd == "quant") in >> q;
            const float init = read_f(in);
            uint32_t h[R2_BINS];
            for (uint32_t &v : h) in >> v;
            if (cmd == "quant") {
                int bin = -1;
                const float r2 = quantile_radius2(h, init, q, &bin);
                printf("quant %d %08x\n", bin, u_of(r2));
            } else {
                r.landed(h, init);
                printf("landed"), state(r);
            }
        } else if (cmd == "bands") {
            long long n = 0, unit = 0;
            int world = 0;
            in >> n >> unit >> world;
            const auto owned = device_bands(n, unit, world);
            printf("bands ");
            for (size_t d = 0; d < owned.size(); ++d) {
                if (d) printf("|");
                for (size_t i = 0; i < owned[d].size(); ++i)
                    printf("%s%" PRId64 ":%" PRId64, i ? "," : "", owned[d][i].first, owned[d][i].second);
            }
            printf("\n");
        } else if (cmd == "new") {
            r = R2Plan();
            in >> r.quantile;
            printf("new"), state(r);
        } else if (cmd == "active") {
            int est = 0;
            in >> est;
            printf("active %d", r.active(est)), state(r);
        } else if (cmd == "due") {
            printf("due %d", r.reduce_due()), state(r);
        } else if (cmd == "issued") {
            r.reduce_issued(stream_of(in));
            printf("issued"), state(r);
        } else if (cmd == "began") {
            int fresh = 0;
            in >> fresh;
            r.pass_began(fresh != 0);
            printf("began"), state(r);
        } else if (cmd == "radius") {
            const float init = read_f(in);
            int fresh = 0;
            in >> fresh;
            printf("radius %08x", u_of(r.radius2(init, fresh != 0))), state(r);
        } else if (cmd == "bin") {
            const float init = read_f(in);
            const R2Plan::BinPrep b = r.before_bin(init, stream_of(in));
            printf("bin wait=%d clear=%d", b.wait, b.clear), state(r);
        } else if (cmd == "binned") {
            r.binned(read_f(in));
            printf("binned"), state(r);
        } else if (cmd == "invalidate") {
            r.invalidate();
            printf("invalidate"), state(r);
        } else {
            fprintf(stderr, "unknown command: %s\n", line.c_str());
            return 1;
        }
        if (!in) { fprintf(stderr, "short command: %s\n", line.c_str()); return 1; }
    }
    return 0;
}
