// hyst_uf_host.cpp -- csrc/hyst_uf.hpp, the union-find core of the hysteresis without a host wait, on the CPU: the four
// phases over crafted masks, on one thread and on eight, against a plain breadth-first flood.  Needs no GPU; exits non-zero
// on the first difference.  tests/test_hyst_uf_host.py builds it plain and with the address and undefined-behaviour
// sanitizers.  The eight threads take the words interleaved (word i goes to thread i mod 8), so neighbouring runs are
// united by different threads at the same time, and every phase is joined before the next one starts, which is what the
// kernel boundaries do on the device.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <queue>
#include <string>
#include <thread>
#include <vector>

#include "../../introtocomputervision_amd/csrc/hyst_uf.hpp"

namespace hy = micv::hyst;

struct HostAtomics {
    static uint32_t load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    static uint32_t fetch_min(uint32_t *p, uint32_t v) {
        uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (v < old && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
        }
        return old;
    }
    static uint32_t ld(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    static void st(uint32_t *p, uint32_t v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
};

struct Mask {
    std::string name;
    int rows, cols;
    std::vector<uint8_t> cand, strong;
    Mask(std::string n, int r, int c) : name(std::move(n)), rows(r), cols(c), cand((size_t)r * c, 0), strong((size_t)r * c, 0) {}
    uint8_t &c(int y, int x) { return cand[(size_t)y * cols + x]; }
    uint8_t &s(int y, int x) { return strong[(size_t)y * cols + x]; }
};

// every component of cand | strong that holds a strong pixel, 8-connected
static std::vector<uint8_t> flood(const Mask &m) {
    const int R = m.rows, C = m.cols;
    std::vector<uint8_t> out((size_t)R * C, 0);
    std::queue<int> q;
    for (int i = 0; i < R * C; i++)
        if (m.strong[i]) {
            out[i] = 255;
            q.push(i);
        }
    while (!q.empty()) {
        const int i = q.front(), y = i / C, x = i % C;
        q.pop();
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int yy = y + dy, xx = x + dx;
                if (yy < 0 || yy >= R || xx < 0 || xx >= C) continue;
                const int j = yy * C + xx;
                if (!out[j] && (m.cand[j] || m.strong[j])) {
                    out[j] = 255;
                    q.push(j);
                }
            }
    }
    return out;
}

static std::vector<uint8_t> union_find(const Mask &m, int nthreads, bool reversed) {
    const int R = m.rows, C = m.cols, T = (C + 63) / 64, nwords = R * T;
    std::vector<uint64_t> F(nwords, 0), S(nwords, 0);
    for (int y = 0; y < R; y++)
        for (int x = 0; x < C; x++) {
            const size_t i = (size_t)y * C + x;
            if (m.cand[i] || m.strong[i]) F[y * T + x / 64] |= 1ull << (x % 64);
            if (m.strong[i]) S[y * T + x / 64] |= 1ull << (x % 64);
        }
    // exactly rows * cols slots, filled with a value no phase may ever meet: a read of a slot that is no run start, or
    // past the end, shows up as a difference or under the address sanitizer
    std::vector<uint32_t> parent((size_t)R * C, 0xDEADBEEFu);
    uint32_t *P = parent.data();
    std::vector<uint8_t> out((size_t)R * C, 0);
    auto phase = [&](const std::function<void(int, int, int)> &body) {
        auto part = [&](int t) {
            for (int k = t; k < nwords; k += nthreads) {
                const int w = reversed ? nwords - 1 - k : k;
                body(w, w / T, w % T);
            }
        };
        if (nthreads == 1) return part(0);
        std::vector<std::thread> pool;
        for (int t = 0; t < nthreads; t++) pool.emplace_back(part, t);
        for (auto &th : pool) th.join();
    };
    auto id0 = [&](int y, int tx) { return (uint32_t)(y * C + tx * 64); };
    phase([&](int w, int y, int tx) { hy::init_word<HostAtomics>(P, F[w], id0(y, tx)); });
    phase([&](int w, int y, int tx) {
        const bool l = tx > 0, r = tx + 1 < T, u = y > 0;
        hy::union_word<HostAtomics>(P, F[w], l ? F[w - 1] : 0, u && l ? F[w - T - 1] : 0, u ? F[w - T] : 0, u && r ? F[w - T + 1] : 0,
                                    id0(y, tx), (uint32_t)C);
    });
    phase([&](int w, int y, int tx) { hy::mark_word<HostAtomics>(P, F[w], S[w], id0(y, tx)); });
    phase([&](int w, int y, int tx) {
        for (int b = 0; b < 64 && tx * 64 + b < C; b++)
            if ((F[w] >> b & 1) && hy::kept_bit<HostAtomics>(P, F[w], id0(y, tx), b)) out[(size_t)y * C + tx * 64 + b] = 255;
    });
    return out;
}

static uint64_t rng_state;
static double uniform() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (double)((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

static Mask serpentine(int R, int C) {  // a one-pixel path: every other row full, joined at alternating ends; strong at the far end
    Mask m("serpentine", R, C);
    int last_y = 0;
    for (int y = 0; y < R; y += 2) {
        for (int x = 0; x < C; x++) m.c(y, x) = 1;
        if (y + 2 < R) m.c(y + 1, (y / 2) % 2 ? 0 : C - 1) = 1;
        last_y = y;
    }
    m.s(last_y, (last_y / 2) % 2 ? 0 : C - 1) = 1;
    return m;
}

static std::vector<Mask> masks() {
    std::vector<Mask> v;
    const int shapes[][2] = {{1, 1}, {1, 200}, {200, 1}, {2, 63}, {2, 64}, {2, 65}, {2, 129}, {63, 63}, {63, 64}, {63, 65},
                             {63, 129}, {64, 63}, {64, 64}, {64, 65}, {64, 129}};
    for (auto &sh : shapes) {
        const int R = sh[0], C = sh[1];
        Mask all("all candidates, one strong", R, C);  // (d)
        for (auto &b : all.cand) b = 1;
        all.s(R - 1, C - 1) = 1;
        v.push_back(all);
        Mask none("candidates, no strong", R, C);
        for (auto &b : none.cand) b = 1;
        v.push_back(none);
        v.push_back(Mask("nothing set", R, C));
        Mask outside("a strong pixel outside cand", R, C);
        for (int x = 0; x + 1 < C; x++) outside.c(0, x) = 1;
        outside.c(0, C - 1) = 0;
        outside.s(0, C - 1) = 1;
        v.push_back(outside);
        Mask diag("diagonals", R, C);  // (b) only diagonal contacts
        for (int y = 0; y < R; y++) {
            if (y < C) diag.c(y, y) = 1;
            if (C - 1 - y >= 0) diag.c(y, C - 1 - y) = 1;
        }
        diag.s(0, 0) = 1;
        v.push_back(diag);
        Mask checker("checkerboard", R, C);
        for (int y = 0; y < R; y++)
            for (int x = 0; x < C; x++) checker.c(y, x) = (x + y) % 2 == 0;
        checker.s(R - 1, (R - 1) % 2 ? (C > 1 ? 1 : 0) : 0) = 1;
        v.push_back(checker);
        v.push_back(serpentine(R, C));
        for (int seed = 0; seed < 2; seed++) {
            Mask rnd("random 0.42", R, C);
            rng_state = 1000 * R + C + seed;
            for (auto &b : rnd.cand) b = uniform() < 0.42;
            for (int k = 0; k < 3; k++) rnd.s((int)(uniform() * R), (int)(uniform() * C)) = 1;
            v.push_back(rnd);
        }
    }
    v.push_back(serpentine(65, 129));  // (a)
    Mask d("diagonal through x = 63 / 64", 130, 130);
    for (int i = 0; i < 130; i++) d.c(i, i) = 1;
    d.s(129, 129) = 1;
    v.push_back(d);
    for (double density : {0.38, 0.42, 0.46})  // (c)
        for (int seed = 0; seed < 4; seed++) {
            Mask rnd("random " + std::to_string(density), 130, 200);
            rng_state = seed + (uint64_t)(density * 100) * 7919;
            for (auto &b : rnd.cand) b = uniform() < density;
            for (int k = 0; k < 3; k++) rnd.s((int)(uniform() * 130), (int)(uniform() * 200)) = 1;
            v.push_back(rnd);
        }
    return v;
}

int main() {
    int checked = 0;
    for (const Mask &m : masks()) {
        const std::vector<uint8_t> want = flood(m);
        for (int run = 0; run < 6; run++) {
            const int threads = run < 2 ? 1 : 8;
            if (union_find(m, threads, run & 1) != want) {
                std::printf("hyst_uf_host: %s %d x %d differs from the flood on %d thread(s)\n", m.name.c_str(), m.rows, m.cols, threads);
                return 1;
            }
            checked++;
        }
    }
    std::printf("hyst_uf_host: ok, %d runs\n", checked);
    return 0;
}
