// ransac_sampler_ref.cpp -- the reference's sampling calls, literally (ps4_cpp/lib/RANSAC.cpp:11-13,
// 20-25,39-40,53 and ps4_cpp/lib/Config.cpp:85-99): a std::seed_seq from the hex words of
// `mersenne_seed` (or seed_seq({1}) without one), one file-static std::mt19937 seeded once, and per
// solve a fresh iota vector that every iteration std::shuffle's in place.
//   ransac_sampler_ref "<hex words>|default" n1 it1 [n2 it2 ...]
// prints, for each solve s, it_s lines: "s i p0 p1 ... p(n_s - 1)", the vector after iteration i.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <numeric>
#include <random>
#include <sstream>
#include <string>
#include <vector>

static std::mt19937 rng;
static bool seeded = false;

static void seed(std::shared_ptr<std::seed_seq> seq) {
    if (!seeded) {
        rng.seed(*seq);
        seeded = true;
    }
}

int main(int argc, char **argv) {
    if (argc < 2 || (argc - 2) % 2) return 2;
    std::shared_ptr<std::seed_seq> mersenneSeed;
    if (std::string(argv[1]) != "default") {
        std::istringstream seedString(argv[1]);
        uint32_t i;
        std::vector<uint32_t> seedVals;
        while (seedString >> std::hex >> i) seedVals.push_back(i);
        mersenneSeed = std::make_shared<std::seed_seq>(seedVals.begin(), seedVals.end());
    } else {
        mersenneSeed = std::unique_ptr<std::seed_seq>(new std::seed_seq({1}));
    }
    seed(mersenneSeed);
    seed(std::shared_ptr<std::seed_seq>(new std::seed_seq({7, 7})));  // ignored, as every later call is
    for (int s = 0; 2 + 2 * s < argc; s++) {
        const size_t numPts = std::strtoul(argv[2 + 2 * s], nullptr, 10);
        const int iters = std::atoi(argv[3 + 2 * s]);
        std::vector<int> indices(numPts);
        std::iota(indices.begin(), indices.end(), 0);
        for (int it = 0; it < iters; it++) {
            std::shuffle(indices.begin(), indices.end(), rng);
            std::printf("%d %d", s, it);
            for (int v : indices) std::printf(" %d", v);
            std::printf("\n");
        }
    }
    return 0;
}
