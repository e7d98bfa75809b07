// TEST HARNESS: the goal curriculum's window, row and level rule (csrc/env_goal.hpp: rbg::curriculum_hi, curriculum_row,
// curriculum_next_level - the functions goal_curriculum_kernel calls) compiled for the host.  A stand-alone program: every line of
// standard input "m L l reached up down seed gid draw" gives a line "hi k next" (k at level l, next: the level after an episode end
// with that outcome).  tests/test_goal_curriculum_cpu.py compares the output with its numpy restatement.
#include <cinttypes>
#include <cstdio>

#include "env_goal.hpp"

int main() {
    uint64_t m, L, l, reached, up, down, seed, gid, draw;
    long lines = 0;
    while (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64,
                      &m, &L, &l, &reached, &up, &down, &seed, &gid, &draw) == 9) {
        const uint32_t hi = rbg::curriculum_hi(uint32_t(l), uint32_t(m), uint32_t(L));
        const uint32_t k = rbg::curriculum_row(seed, gid, uint32_t(draw), uint32_t(l), uint32_t(m), uint32_t(L));
        const uint32_t next = rbg::curriculum_next_level(uint32_t(l), reached != 0, uint32_t(up), uint32_t(down), uint32_t(L));
        std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", hi, k, next);
        ++lines;
    }
    return lines ? 0 : 1;
}
