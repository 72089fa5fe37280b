// hyst_uf.hpp -- the union-find core of the hysteresis that needs no host (canny_uf.hip), in plain C++ that compiles for
// the host as well as the device: it includes the standard headers only, so tests/cpp/hyst_uf_host.cpp runs it on the CPU,
// on one thread and on eight, under the address and undefined-behaviour sanitizers against a plain flood.
//
// 8-connected hysteresis keeps every component of F = weak | strong that holds a strong pixel: connected-component
// labelling.  The planes are bit planes, one 64-bit word per (row, 64 columns), bit b = column 64 * tx + b.
//   element   a maximal horizontal run of F bits inside ONE word (a run that crosses a word edge is two elements)
//   id        the pixel index y * cols + x of the run's first bit, < 2^31
//   parent    P[id], a u32 plane with one slot per pixel; only slots of run starts are ever written or read, so the plane
//             needs no clearing
// Four phases, each complete before the next begins (a kernel boundary on the device, a join in the host program):
//   init_word    every run of the word: P[id] = id
//   union_word   every run of the word is united with the run that ends at bit 63 of the word to its left (when it starts at
//                bit 0) and with every run of the row above that meets columns [s - 1, e + 1] -- bit 63 of the upper-left
//                word and bit 0 of the upper-right word included.  Up and left suffice: every adjacency is seen from its
//                lower or its right element.
//   mark_word    every run jumps to its root (flatten), and one that holds a strong bit stores kMarked over the root's parent
//   kept_bit     a pixel is an edge when the root of its run is marked
//
// THE LOOPS END without help from any other thread.  During the union phase a slot is only ever changed by fetch_min, so it
// only decreases, and P[x] <= x always (init stores x).  walk() steps from x to P[x] < x; compress() steps from x to the
// parent x had, < x; unite() goes round again only with a = the parent a had, < a.  Each iteration strictly lowers a value
// bounded below by 0.  Nothing waits for a store that somebody else has yet to make.
//
// THE RESULT IS RIGHT whatever the interleaving, and whatever stale value a load returns.  Call two nodes joined when a
// path of current parent links and of DEBTS connects them; a debt is a pair a thread still holds: the (a, b) of a running
// unite(), the (x, r) of a running compress().  Every step keeps joined nodes joined:
//   * a load of P[a] gives p, and the thread goes on with p in a's place: a - p is a link, or was one, and joined nodes
//     stay joined, so (p, b) serves as (a, b) did.
//   * old = fetch_min(&P[a], b) for a debt (a, b), a > b.  old == a: a was a root and is now linked to b; the debt is paid.
//     b < old: the link a - old is replaced by a - b, which pays (a, b), and the thread takes on (old, b), so old stays
//     joined to a through b.  b >= old: nothing changed; a - old is a link, so (old, b) serves as (a, b) did.
//   The decision rests on the value the read-modify-write returns, never on a load.  unite() returns only with its debt
//   paid or with both ends at one node.  compress() pays or hands on its debt the same way while old > r; when it meets
//   old < r (r has stopped being a root) beyond its first step, it owes (old, r) and pays it by a unite() that does not
//   compress.  On its first step it owes nothing: x was joined to r before.
// When the phase ends no debt is left, so links alone join whatever a unite() was called for: every adjacency.  Links
// are only ever made between nodes some unite() was owed for, so nothing else is joined.
//
// A is the tiny wrapper that holds the memory operations: load / fetch_min are the union phase's (atomic, device-wide),
// ld / st the other phases' (plain on the device; several threads store the same kMarked).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define MICV_HD __host__ __device__
#else
#define MICV_HD
#endif

namespace micv {
namespace hyst {

constexpr uint32_t kMarked = 0xFFFFFFFFu;  // never an id: ids are below 2^31

// bits s..e of a word, 0 <= s <= e <= 63
MICV_HD inline uint64_t span(int s, int e) { return (~0ull >> (63 - e)) & (~0ull << s); }
// the first and the last bit of the run of F that holds its set bit b
MICV_HD inline int run_start(uint64_t F, int b) {
    const uint64_t gaps = ~F & ((1ull << b) - 1);
    return gaps ? 64 - __builtin_clzll(gaps) : 0;
}
MICV_HD inline int run_end(uint64_t F, int b) {
    const uint64_t gaps = ~F >> b;  // bit 0 is clear: b is set in F
    return gaps ? b + __builtin_ctzll(gaps) - 1 : 63;
}
// fn(s, e) for every run of F, lowest first
template <typename Fn>
MICV_HD inline void for_each_run(uint64_t F, Fn fn) {
    while (F) {
        const int s = __builtin_ctzll(F), e = run_end(F, s);
        fn(s, e);
        F &= ~span(s, e);
    }
}

template <typename A>
MICV_HD inline uint32_t walk(uint32_t *P, uint32_t x) {
    for (uint32_t p; (p = A::load(P + x)) != x;) x = p;
    return x;
}

template <typename A, bool Compress>
MICV_HD inline void unite(uint32_t *P, uint32_t a, uint32_t b);

// every node on the way from x re-parented to r, the root walk(x) gave
template <typename A>
MICV_HD inline void compress(uint32_t *P, uint32_t x, uint32_t r) {
    for (bool first = true; x > r; first = false) {
        const uint32_t old = A::fetch_min(P + x, r);
        if (old == x) return;  // a root until now: linked, paid
        if (old < r && !first) unite<A, false>(P, r, old);
        x = old;
    }
}

template <typename A, bool Compress>
MICV_HD inline uint32_t find(uint32_t *P, uint32_t x) {
    const uint32_t r = walk<A>(P, x);
    if (Compress) compress<A>(P, x, r);
    return r;
}

template <typename A, bool Compress>
MICV_HD inline void unite(uint32_t *P, uint32_t a, uint32_t b) {
    for (;;) {
        a = find<A, Compress>(P, a);
        b = find<A, Compress>(P, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = A::fetch_min(P + a, b);
        if (old == a) return;  // a was a root until this very operation
        a = old;               // it was not: its former parent takes its place
    }
}

template <typename A>
MICV_HD inline void init_word(uint32_t *P, uint64_t F, uint32_t id0) {
    for_each_run(F, [&](int s, int) { A::st(P + id0 + s, id0 + s); });
}

// F: this word, id0 the id of its bit 0; left: the word to its left; ul, uc, ur: the three words above.  A word that
// does not exist is passed as 0.
template <typename A>
MICV_HD inline void union_word(uint32_t *P, uint64_t F, uint64_t left, uint64_t ul, uint64_t uc, uint64_t ur, uint32_t id0,
                               uint32_t cols) {
    const uint32_t up0 = id0 - cols;  // used only when a word above exists
    for_each_run(F, [&](int s, int e) {
        const uint32_t me = id0 + s;
        if (s == 0 && left >> 63) unite<A, true>(P, me, id0 - 64 + run_start(left, 63));
        if (s == 0 && ul >> 63) unite<A, true>(P, me, up0 - 64 + run_start(ul, 63));
        uint64_t m = uc & span(s > 0 ? s - 1 : 0, e < 63 ? e + 1 : 63);
        while (m) {
            const int b = __builtin_ctzll(m), us = run_start(uc, b);
            unite<A, true>(P, me, up0 + us);
            m &= ~span(us, run_end(uc, b));
        }
        if (e == 63 && (ur & 1)) unite<A, true>(P, me, up0 + 64);
    });
}

// after the union phase: nothing moves but root -> kMarked
template <typename A>
MICV_HD inline uint32_t root(const uint32_t *P, uint32_t x) {
    for (;;) {
        const uint32_t p = A::ld(P + x);
        if (p == x || p == kMarked) return x;
        x = p;
    }
}

// The root of x by pointer jumping: x is re-parented to its grandparent until its parent is a root.  Concurrent union
// leaves chains (a vertical line of one-pixel runs, each linked to the one above while all were roots, is a chain as deep
// as the line is tall); with every run jumping at once a chain of depth d is flat after about log2 d steps of each, where
// root() alone would walk d links.  Each step stores a smaller value over P[x], so the loop ends by itself; a racing
// reader sees the old parent or the new one, both ancestors.  kMarked is never stored over anything but a root.
template <typename A>
MICV_HD inline uint32_t flatten(uint32_t *P, uint32_t x) {
    for (;;) {
        const uint32_t p = A::ld(P + x);
        if (p == x || p == kMarked) return x;
        const uint32_t g = A::ld(P + p);
        if (g == p || g == kMarked) return p;
        A::st(P + x, g);
    }
}

// every run is left pointing at its root; a run that holds a strong bit marks that root
template <typename A>
MICV_HD inline void mark_word(uint32_t *P, uint64_t F, uint64_t S, uint32_t id0) {
    for_each_run(F, [&](int s, int e) {
        const uint32_t r = flatten<A>(P, id0 + s);
        if (S & span(s, e)) A::st(P + r, kMarked);
    });
}

// after the mark phase: is the set bit b of F kept?
template <typename A>
MICV_HD inline bool kept_bit(const uint32_t *P, uint64_t F, uint32_t id0, int b) {
    return A::ld(P + root<A>(P, id0 + run_start(F, b))) == kMarked;
}

}  // namespace hyst
}  // namespace micv
