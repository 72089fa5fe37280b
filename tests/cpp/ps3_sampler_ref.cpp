// ps3_sampler_ref.cpp -- the sampling calls of ps3's trial loop, in standard-library calls only: a std::seed_seq
// from the hex words of `mersenne_seed` (or seed_seq({1}) without one) seeds one std::mt19937; every trial fills a
// FRESH vector with 0 .. n-1 (std::iota) and std::shuffle's it with that engine.
//   ps3_sampler_ref "<hex words>|default" n1 trials1 [n2 trials2 ...]
// prints, for each run s, trials_s lines "s t p0 p1 ... p(n_s - 1)".  The engine runs through all of them, so a later
// run pins the state the earlier ones left.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <sstream>
#include <string>
#include <vector>

int main(int argc, char **argv) {
    if (argc < 4 || (argc - 2) % 2) return 2;
    std::vector<uint32_t> words;
    if (std::string(argv[1]) != "default") {
        std::istringstream in(argv[1]);
        uint32_t w;
        while (in >> std::hex >> w) words.push_back(w);
    } else {
        words.push_back(1);
    }
    std::seed_seq seq(words.begin(), words.end());
    std::mt19937 engine;
    engine.seed(seq);
    for (int s = 0; 2 + 2 * s < argc; s++) {
        const size_t n = std::strtoul(argv[2 + 2 * s], nullptr, 10);
        const int trials = std::atoi(argv[3 + 2 * s]);
        for (int t = 0; t < trials; t++) {
            std::vector<int> nums(n);
            std::iota(nums.begin(), nums.end(), 0);
            std::shuffle(nums.begin(), nums.end(), engine);
            std::printf("%d %d", s, t);
            for (int v : nums) std::printf(" %d", v);
            std::printf("\n");
        }
    }
    return 0;
}
