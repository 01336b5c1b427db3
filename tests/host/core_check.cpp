// Host check of marl-hideandseek_amd/csrc/hs_core_probe.h (tests/test_core_float64.py builds and runs it): the scalar
// core's probe table in a stand-alone program, so that the address and undefined-behaviour sanitizers can watch the core's
// arithmetic (signed ranges of sampleI32, the float-to-int conversion of the trigonometry's reduction, shifts of the RNG).
//   core_check file PATH     PATH holds records of 17 32-bit words: op, then the 16 input words of one case.
// Prints, for every op that occurs, the number of cases and a checksum of all their output words in file order:
//   sum over i of (word_i + 0x9E3779B97F4A7C15) * (2 i + 1)  mod 2^64,   i counting the op's output words from 0,
// which the test recomputes from the oracle's hsref_core_eval on the same inputs.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hs_core_probe.h"

int main(int argc, char **argv) {
    if (argc != 3 || std::strcmp(argv[1], "file") != 0) { std::fprintf(stderr, "usage: core_check file PATH\n"); return 2; }
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    std::vector<uint64_t> sum(hs::CORE_NUM_OPS, 0), words(hs::CORE_NUM_OPS, 0), cases(hs::CORE_NUM_OPS, 0);
    uint32_t rec[1 + hs::kCoreWords];
    size_t got;
    while ((got = std::fread(rec, 4, 1 + hs::kCoreWords, f)) == (size_t)(1 + hs::kCoreWords)) {
        const int32_t op = (int32_t)rec[0];
        if (op < 0 || op >= hs::CORE_NUM_OPS) { std::fprintf(stderr, "unknown op %d\n", op); return 1; }
        float in[hs::kCoreWords], out[hs::kCoreWords];
        std::memcpy(in, rec + 1, sizeof(in));
        hs::core_eval(op, in, out);
        for (int k = 0; k < hs::kCoreWords; ++k) {
            uint32_t w;
            std::memcpy(&w, &out[k], 4);
            sum[op] += ((uint64_t)w + 0x9E3779B97F4A7C15ull) * (2 * words[op] + 1);
            ++words[op];
        }
        ++cases[op];
    }
    std::fclose(f);
    if (got != 0) { std::fprintf(stderr, "truncated record\n"); return 1; }
    for (int op = 0; op < hs::CORE_NUM_OPS; ++op)
        if (cases[op]) std::printf("op %d cases %" PRIu64 " checksum %016" PRIx64 "\n", op, cases[op], sum[op]);
    std::printf("file OK\n");
    return 0;
}
