// TEST HARNESS: the episode log's lane rule (csrc/env_episode_log.hpp: rbel::lane_step, the function the kernel calls) built for the
// host and driven over recorded sequences, with the planes laid out and indexed as the kernel's are ([n] and [E][n], exactly sized, so
// a sanitizer build sees every index).  stdin:  n E T,  then n words: the counters `seen` starts from,  then T blocks of n lines
// "reward-bits done reached".  stdout: n lines "count acc-bits age seen", E * n lines "ret-bits len kind" (plane-major), one line "full".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "env_episode_log.hpp"

int main() {
    long n = 0, T = 0;
    unsigned E = 0;
    if (std::scanf("%ld %u %ld", &n, &E, &T) != 3 || n < 1 || E < 1 || E > unsigned(rbel::MAX_CAPACITY) || T < 0) return 2;
    std::vector<float> acc(n, 0.0f), ret(size_t(E) * n, 0.0f);
    std::vector<uint32_t> age(n, 0u), seen(n, 0u), count(n, 0u), len(size_t(E) * n, 0u), kind(size_t(E) * n, 0u);
    uint32_t full = 0;
    for (long i = 0; i < n; ++i)
        if (std::scanf("%u", &seen[i]) != 1) return 2;
    for (long t = 0; t < T; ++t)
        for (long i = 0; i < n; ++i) {
            uint32_t bits, done, reached;
            if (std::scanf("%u %u %u", &bits, &done, &reached) != 3) return 2;
            float r;
            std::memcpy(&r, &bits, 4);
            rbel::Lane s{acc.at(i), age.at(i), seen.at(i), count.at(i)};
            const rbel::Record rec = rbel::lane_step(s, r, done, reached, E);
            acc.at(i) = s.acc; age.at(i) = s.age; seen.at(i) = s.seen; count.at(i) = s.count;
            if (rec.slot != rbel::NO_SLOT) {
                const size_t at = size_t(rec.slot) * size_t(n) + size_t(i);
                ret.at(at) = rec.ret; len.at(at) = rec.len; kind.at(at) = rec.kind;
                if (rec.filled) ++full;
            }
        }
    for (long i = 0; i < n; ++i) {
        uint32_t bits;
        std::memcpy(&bits, &acc[i], 4);
        std::printf("%u %u %u %u\n", count[i], bits, age[i], seen[i]);
    }
    for (size_t at = 0; at < size_t(E) * n; ++at) {
        uint32_t bits;
        std::memcpy(&bits, &ret[at], 4);
        std::printf("%u %u %u\n", bits, len[at], kind[at]);
    }
    std::printf("%u\n", full);
    return 0;
}
