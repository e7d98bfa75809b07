// TEST HARNESS: the start poses' decision, row and counter (csrc/env_start.hpp: rbstart::start_draw - the function env_start calls)
// compiled for the host.  A stand-alone program: every line of standard input "seed gid d threshold m" gives a line "index count"
// (index: the pool row, or 4294967295 for the rest pose; count: the counter behind the start).  tests/test_start_poses_cpu.py compares
// the output with its numpy restatement.
#include <cinttypes>
#include <cstdio>

#include "env_start.hpp"

int main() {
    uint64_t seed, gid, d, threshold, m;
    long lines = 0;
    while (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &seed, &gid, &d, &threshold, &m) == 5) {
        const rbstart::Start st = rbstart::start_draw(seed, gid, uint32_t(d), uint32_t(threshold), uint32_t(m));
        std::printf("%" PRIu32 " %" PRIu32 "\n", st.index, st.count);
        ++lines;
    }
    return lines ? 0 : 1;
}
