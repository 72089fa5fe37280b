// match.hip -- descriptor matching of ps4: brute-force 2-nearest
// neighbours under L2 and the Lowe ratio test (cv::BFMatcher::knnMatch(k=2) + `d0 < 0.75 d1`,
// ps4_cpp/src/Solution.cpp:172-184).
//
// N x M x dim squared differences look like a GEMM, and ||a-b||^2 = ||a||^2 + ||b||^2 - 2ab would
// put it on MFMA -- but that changes every low-order bit (cancellation) and with it the ranking of
// near-ties.  The contract is the direct form, one fmaf chain per (query, train) pair in dimension
// order, so this is an LDS-tiled VALU kernel: a workgroup owns 64 queries, streams the train set
// through LDS in tiles of 64 rows, and every thread carries 16 independent chains (one query x 16
// train rows), reading its query element from a padded LDS image and the train element as a
// wave-wide broadcast.
#include <algorithm>

#include "compact.hpp"
#include "kernels.hpp"

namespace micv {

struct Top2 {
    float d0, d1;
    int i0, i1;
    __device__ void init() { d0 = d1 = INFINITY; i0 = i1 = -1; }
    // order by (distance, index): what a strict `<` scan in index order keeps
    __device__ void push(float d, int i) {
        if (d < d0 || (d == d0 && (unsigned)i < (unsigned)i0)) {
            d1 = d0; i1 = i0; d0 = d; i0 = i;
        } else if (d < d1 || (d == d1 && (unsigned)i < (unsigned)i1)) {
            d1 = d; i1 = i;
        }
    }
};

// Tile: 64 queries x 128 train rows per pass of a 256-thread workgroup, a thread owns 4 queries x 8
// train rows (32 chains).  Both operands are staged TRANSPOSED ([k][row]) so that a thread's 4
// query values and 8 train values of one dimension k are ds_read_b128 reads, and adjacent train
// rows sit in adjacent registers: the chain step  d = a - t; acc = fma(d, d, acc)  runs as
// v_pk_add_f32 / v_pk_fma_f32 on (t_j, t_j+1) pairs -- two chains per instruction, each still its
// own IEEE fmaf chain in dimension order.  The train set is cut into slices over blockIdx.y so
// that small query sets still fill the GPU; bf_merge_kernel folds the slices' top-2 in slice
// (= index) order.
typedef float mf2 __attribute__((ext_vector_type(2)));
typedef float mf4 __attribute__((ext_vector_type(4)));
constexpr int kQT = 64, kTT = 128, kDC = 32;

// COUNTED (micv_bf_knn2_counted_dev): nq_cap / nt_cap size the grid, the slices and the partial lists; the lengths
// themselves are device words, clamped to [0, cap].  A workgroup whose queries all lie at or past the count leaves as a whole
// before any barrier; a slice at or past the train count runs no pass and leaves its queries' lists empty.
__device__ __forceinline__ int bf_clamped_count(const int64_t *count, int cap) {
    const int64_t c = *count;
    return c < 0 ? 0 : (c < cap ? (int)c : cap);
}

// The tile body of every search kernel: queries [q0, q0 + 64) of `query` (rows at and past nq are not read) against train
// rows [ts0, ts1).  Returns true in the threads that hold a query's folded top-2 (tid < 64, q0 + tid < nq), `m` is that list.
__device__ __forceinline__ bool bf_tile_search(const float *__restrict__ query, int q0, int nq, int qstride,
                                               const float *__restrict__ train, int ts0, int ts1, int tstride, int dim,
                                               int vec_ok, Top2 &m) {
    __shared__ __attribute__((aligned(16))) float Qt[kDC][kQT];
    __shared__ __attribute__((aligned(16))) float Tt[kDC][kTT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    Top2 best[4];
#pragma unroll
    for (int i = 0; i < 4; i++) best[i].init();
    for (int t0 = ts0; t0 < ts1; t0 += kTT) {
        mf2 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[i][j] = (mf2)(0.f);
        // The next chunk's operands are PREFETCHED into registers (24 floats per thread) before the current chunk's chains
        // run and written to LDS after them: the global round trip flies under 32 x 32 packed instructions instead of in
        // front of them (r05; the same move as the stereo NCC kernel).
        float pq[8], pt[16];
        // (a lane reads 8 / 16 consecutive floats of ITS OWN row, so every load instruction touches 64 different cache
        // lines: as 16-byte loads -- rows and pitches aligned, dim a multiple of 4 -- that is 6 instructions per chunk
        // instead of 24, and the address unit stops being the co-limiter of the chains; r05)
        auto prefetch = [&](int k0) {
            {
                const int r = tid & 63, kq = (tid >> 6) * 8;
                const bool rin = q0 + r < nq;
                const float *src = query + (size_t)(rin ? q0 + r : 0) * qstride + k0 + kq;
                if (vec_ok) {
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const mf4 v = (rin && k0 + kq + 4 * i < dim) ? *reinterpret_cast<const mf4 *>(src + 4 * i) : (mf4)(0.f);
                        pq[4 * i] = v.x; pq[4 * i + 1] = v.y; pq[4 * i + 2] = v.z; pq[4 * i + 3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 8; i++) pq[i] = (rin && k0 + kq + i < dim) ? src[i] : 0.f;
                }
            }
            {
                const int r = tid & 127, kh = (tid >> 7) * 16;
                const bool rin = t0 + r < ts1;
                const float *src = train + (size_t)(rin ? t0 + r : 0) * tstride + k0 + kh;
                if (vec_ok) {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const mf4 v = (rin && k0 + kh + 4 * i < dim) ? *reinterpret_cast<const mf4 *>(src + 4 * i) : (mf4)(0.f);
                        pt[4 * i] = v.x; pt[4 * i + 1] = v.y; pt[4 * i + 2] = v.z; pt[4 * i + 3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 16; i++) pt[i] = (rin && k0 + kh + i < dim) ? src[i] : 0.f;
                }
            }
        };
        prefetch(0);
        for (int k0 = 0; k0 < dim; k0 += kDC) {  // chains continue across chunks in dimension order
            __syncthreads();
            {   // stage, transposing: lane = row, so the LDS stores of one k are contiguous
                const int r = tid & 63, kq = (tid >> 6) * 8;
#pragma unroll
                for (int i = 0; i < 8; i++) Qt[kq + i][r] = pq[i];
            }
            {
                const int r = tid & 127, kh = (tid >> 7) * 16;
#pragma unroll
                for (int i = 0; i < 16; i++) Tt[kh + i][r] = pt[i];
            }
            __syncthreads();
            if (k0 + kDC < dim) prefetch(k0 + kDC);
            const int kn = dim - k0 < kDC ? dim - k0 : kDC;
#pragma unroll 4
            for (int k = 0; k < kn; k++) {
                const mf4 a = *reinterpret_cast<const mf4 *>(&Qt[k][4 * tx]);
                const mf4 b0 = *reinterpret_cast<const mf4 *>(&Tt[k][8 * ty]);
                const mf4 b1 = *reinterpret_cast<const mf4 *>(&Tt[k][8 * ty + 4]);
                const mf2 t[4] = {b0.xy, b0.zw, b1.xy, b1.zw};
                const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const mf2 d = (mf2)(av[i]) - t[j];
                        acc[i][j] = __builtin_elementwise_fma(d, d, acc[i][j]);
                    }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int t = t0 + 8 * ty + 2 * j;
                if (t < ts1) best[i].push(acc[i][j].x, t);
                if (t + 1 < ts1) best[i].push(acc[i][j].y, t + 1);
            }
    }
    // fold the 16 train-row groups of each query (ascending ty = ascending index)
    __shared__ float md[16][kQT][2];
    __shared__ int mi[16][kQT][2];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        md[ty][4 * tx + i][0] = best[i].d0; md[ty][4 * tx + i][1] = best[i].d1;
        mi[ty][4 * tx + i][0] = best[i].i0; mi[ty][4 * tx + i][1] = best[i].i1;
    }
    __syncthreads();
    if (!(tid < kQT && q0 + tid < nq)) return false;
    m.init();
    for (int g = 0; g < 16; g++)
        for (int sidx = 0; sidx < 2; sidx++)
            if (mi[g][tid][sidx] >= 0) m.push(md[g][tid][sidx], mi[g][tid][sidx]);
    return true;
}

template <bool COUNTED>
__global__ __launch_bounds__(256) void bf_knn2_kernel(const float *__restrict__ query, int nq_cap,
                                                       int qstride, const float *__restrict__ train,
                                                       int nt_cap, int tstride, int dim, int slice_rows,
                                                       int32_t *__restrict__ part_i,
                                                       float *__restrict__ part_d, int vec_ok,
                                                       const int64_t *__restrict__ nq_count,
                                                       const int64_t *__restrict__ nt_count) {
    int nq = nq_cap, nt = nt_cap;
    if constexpr (COUNTED) {
        nq = bf_clamped_count(nq_count, nq_cap);
        nt = bf_clamped_count(nt_count, nt_cap);
        if ((int)blockIdx.x * kQT >= nq) return;
    }
    const int q0 = blockIdx.x * kQT;
    const int ts0 = blockIdx.y * slice_rows, ts1 = ts0 + slice_rows < nt ? ts0 + slice_rows : nt;
    Top2 m;
    if (bf_tile_search(query, q0, nq, qstride, train, ts0, ts1, tstride, dim, vec_ok, m)) {
        const size_t o = ((size_t)blockIdx.y * nq_cap + q0 + threadIdx.x) * 2;
        part_i[o] = m.i0; part_i[o + 1] = m.i1;
        part_d[o] = m.d0; part_d[o + 1] = m.d1;
    }
}

// Top-2 over the slices' partial top-2 lists (slice order = index order), then the square roots.
// COUNTED: rows at and past the query count get {-1, -1} and {+inf, +inf} (their partial lists were never written).
template <bool COUNTED>
__global__ __launch_bounds__(256) void bf_merge_kernel(const int32_t *__restrict__ part_i,
                                                        const float *__restrict__ part_d, int nq,
                                                        int slices, int32_t *__restrict__ idx2,
                                                        float *__restrict__ dist2, const int64_t *__restrict__ nq_count) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    Top2 m;
    m.init();
    if constexpr (COUNTED) {
        if (q >= bf_clamped_count(nq_count, nq)) slices = 0;
    }
    for (int s = 0; s < slices; s++)
        for (int k = 0; k < 2; k++) {
            const size_t o = ((size_t)s * nq + q) * 2 + k;
            if (part_i[o] >= 0) m.push(part_d[o], part_i[o]);
        }
    idx2[2 * q] = m.i0;
    idx2[2 * q + 1] = m.i1;
    dist2[2 * q] = sqrtf(m.d0);
    dist2[2 * q + 1] = sqrtf(m.d1);
}

struct RatioPred {
    const float *dist2;
    double ratio;
    // (center / test: the one-launch compaction loads a thread's 16 pairs before it decides the first, compact.hpp)
    __device__ float2 center(int64_t q) const { return make_float2(dist2[2 * q], dist2[2 * q + 1]); }  // (caller's pointer: 4-byte aligned)
    __device__ bool test(int64_t, float2 d) const { return (double)d.x < ratio * (double)d.y; }  // Solution.cpp:181
    __device__ bool operator()(int64_t q) const { return test(q, center(q)); }
};

__global__ void bf_emit_kernel(const int32_t *__restrict__ sel, const int64_t *__restrict__ count,
                               int64_t cap, const int32_t *__restrict__ idx2,
                               const float *__restrict__ dist2, int32_t *__restrict__ matches,
                               float *__restrict__ distances) {
    const int64_t n = *count < cap ? *count : cap;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int q = sel[i];
        matches[2 * i] = q;
        matches[2 * i + 1] = idx2[2 * q];
        distances[i] = dist2[2 * q];
    }
}

// ---- a batch of pairs (micv_bf_match_pairs_dev) ----
// Two launches for a whole piece of the batch, the pair a grid dimension of both; neither waits for the host.
//   bf_knn2_pairs_kernel    the tile body above on (64-query block, train slice, pair)
//   bf_finish_pairs_kernel  ONE workgroup per pair: folds the slices, takes the roots, writes idx2 / dist2, applies the
//                           ratio test and compacts in query order with wave ballots and a carried base -- no workgroup
//                           waits for another, no status words, no compact_state slot (harris_list_kernel's pattern)
// SLICING.  The launch has S = gridDim.y slices; how many train rows a slice holds is decided ON THE DEVICE from the
// pair's clamped train count nt:  slice_rows = ceil(ceil(nt / 128) / S) * 128, slice s = rows [s * slice_rows,
// min((s + 1) * slice_rows, nt)), so ceil(nt / slice_rows) slices hold rows and a short list still spreads over as
// many workgroups as it has 128-row passes.  Workgroups of the other slices, and of query blocks at and past the query
// count, leave before any barrier and write nothing; the finish kernel derives the same numbers and reads only what was
// written.  The top-2 order (distance, index) is total, so no output depends on S.
constexpr size_t kPairsScratchBytes = size_t(64) << 20;  // partial lists of one piece (mi_cv.h)
constexpr int kPairsWantWgs = 2048;                      // S: enough slices for this many workgroups, at most cap / 128
constexpr int kFinishThreads = 1024;

struct alignas(16) PairPart {  // one query's top-2 within one slice
    int i0, i1;
    float d0, d1;
};

__device__ __forceinline__ int bf_pair_slice_rows(int nt, int slices) {
    const int passes = (nt + kTT - 1) / kTT;
    return (passes + slices - 1) / slices * kTT;
}

// The lists of pair p: false when an image index lies outside [0, images) (two empty lists).
__device__ __forceinline__ bool bf_pair_lists(const int32_t *__restrict__ pairs, int p, int images, int cap,
                                              const int64_t *__restrict__ count, int &a, int &b, int &nq, int &nt) {
    a = pairs[2 * (size_t)p];
    b = pairs[2 * (size_t)p + 1];
    nq = nt = 0;
    if ((unsigned)a >= (unsigned)images || (unsigned)b >= (unsigned)images) return false;
    nq = count ? bf_clamped_count(count + a, cap) : cap;
    nt = count ? bf_clamped_count(count + b, cap) : cap;
    return true;
}

// (the two list pointers are computed here, not kernel arguments the compiler can load again, and two scalar words spill
// into a VGPR lane: without the occupancy attribute that lane is the 129th VGPR and the fourth workgroup per CU is lost)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void bf_knn2_pairs_kernel(const float *__restrict__ desc, int images, size_t image_floats,
                                                             int cap, int dstride, const int64_t *__restrict__ count, int dim,
                                                             const int32_t *__restrict__ pairs, int pair0,
                                                             PairPart *__restrict__ part, int vec_ok) {
    int a, b, nq, nt;
    if (!bf_pair_lists(pairs, pair0 + (int)blockIdx.z, images, cap, count, a, b, nq, nt)) return;
    const int q0 = blockIdx.x * kQT;
    if (q0 >= nq) return;
    part += ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * cap + q0;  // (now: fewer words live across the tile body)
    const int slice_rows = bf_pair_slice_rows(nt, gridDim.y);
    const int ts0 = blockIdx.y * slice_rows, ts1 = ts0 + slice_rows < nt ? ts0 + slice_rows : nt;  // (cap <= 2^30: no overflow)
    if (ts0 >= nt) return;
    Top2 m;
    if (bf_tile_search(desc + a * image_floats, q0, nq, dstride, desc + b * image_floats, ts0, ts1, dstride, dim, vec_ok, m)) {
        part[threadIdx.x] = PairPart{m.i0, m.i1, m.d0, m.d1};
    }
}

__global__ __launch_bounds__(kFinishThreads) void bf_finish_pairs_kernel(const PairPart *__restrict__ part, int images, int cap,
                                                                          const int64_t *__restrict__ count,
                                                                          const int32_t *__restrict__ pairs, int pair0, int slices,
                                                                          double ratio, int32_t *__restrict__ idx2,
                                                                          float *__restrict__ dist2, int32_t *__restrict__ matches,
                                                                          float *__restrict__ distances, int64_t mcap,
                                                                          int64_t *__restrict__ match_count) {
    __shared__ unsigned wave_total[kFinishThreads / 64];
    const size_t p = (size_t)pair0 + blockIdx.x;
    int a, b, nq, nt;
    bf_pair_lists(pairs, (int)p, images, cap, count, a, b, nq, nt);
    const int slice_rows = bf_pair_slice_rows(nt, slices);
    const int used = nt > 0 ? (nt + slice_rows - 1) / slice_rows : 0;
    const size_t part0 = (size_t)blockIdx.x * slices * cap;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t *I = idx2 ? idx2 + p * (size_t)cap * 2 : nullptr;
    float *D = dist2 ? dist2 + p * (size_t)cap * 2 : nullptr;
    int32_t *M = matches + p * (size_t)mcap * 2;  // (never dereferenced when mcap == 0)
    float *E = distances + p * (size_t)mcap;
    int64_t base = 0;
    for (int q0 = 0; q0 < cap; q0 += kFinishThreads) {
        const int q = q0 + (int)threadIdx.x;
        Top2 m;
        m.init();
        if (q < nq)
            for (int s = 0; s < used; s++) {
                const PairPart r = part[part0 + (size_t)s * cap + q];
                if (r.i0 >= 0) m.push(r.d0, r.i0);
                if (r.i1 >= 0) m.push(r.d1, r.i1);
            }
        const float d0 = sqrtf(m.d0), d1 = sqrtf(m.d1);
        if (q < cap && I) {
            I[2 * (size_t)q] = m.i0; I[2 * (size_t)q + 1] = m.i1;
            D[2 * (size_t)q] = d0; D[2 * (size_t)q + 1] = d1;
        }
        const bool keep = q < cap && RatioPred{nullptr, ratio}.test(q, make_float2(d0, d1));
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wave_total[wave] = __popcll(bal);
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int j = 0; j < kFinishThreads / 64; j++) {
            const unsigned t = wave_total[j];
            before += j < wave ? t : 0u;
            total += t;
        }
        __syncthreads();  // wave_total is written again in the next pass
        if (keep) {
            const int64_t pos = base + before + __popcll(bal & ((1ull << lane) - 1));
            if (pos < mcap) {
                M[2 * pos] = q; M[2 * pos + 1] = m.i0;
                E[pos] = d0;
            }
        }
        base += total;
    }
    if (threadIdx.x == 0) match_count[p] = base;
}

}  // namespace micv

using namespace micv;

// Both matcher entries: nq / nt are the lengths (counts null) or the capacities the launch is sized from.
static int bf_knn2_run(micv_ctx *ctx, const float *query, int nq, size_t qstride, const int64_t *nq_count, const float *train, int nt,
                       size_t tstride, const int64_t *nt_count, int dim, int32_t *idx2, float *dist2, micv_stream stream) {
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // slices of the train set: enough workgroups for 2 - 4 per CU, whole 128-row passes per slice
    const int qblocks = (int)cdiv(nq, kQT), passes = (int)cdiv(nt, kTT);
    // (r05: four workgroups per CU once every workgroup still has eight passes to run -- 8192 x 8192: 0.438 -> 0.389 ms;
    // shorter jobs keep two per CU: 5035 x 5035 0.202 against 0.210, 500 x 20000 0.127 against 0.140)
    const int want_wgs = (long long)qblocks * passes >= 8192 ? 1024 : 512;
    int slices = (want_wgs + qblocks - 1) / qblocks;
    if (slices > passes) slices = passes;
    if (slices < 1) slices = 1;
    const int slice_rows = (int)cdiv(passes, slices) * kTT;
    slices = (int)cdiv(nt, slice_rows);
    void *scratch;
    MICV_TRY(ctx->reserve(2 * Carver::need((size_t)slices * nq * 2, 4), &scratch));
    Carver c(scratch);
    int32_t *part_i = c.take<int32_t>((size_t)slices * nq * 2);
    float *part_d = c.take<float>((size_t)slices * nq * 2);
    const int vec_ok = ((reinterpret_cast<uintptr_t>(query) | reinterpret_cast<uintptr_t>(train) | qstride | tstride) & 15) == 0 &&
                       (dim & 3) == 0;
    if (nq_count) {
        bf_knn2_kernel<true><<<dim3(qblocks, slices), 256, 0, s>>>(query, nq, (int)(qstride / 4), train, nt, (int)(tstride / 4), dim,
                                                                   slice_rows, part_i, part_d, vec_ok, nq_count, nt_count);
        MICV_LAUNCH_CHECK();
        bf_merge_kernel<true><<<cdiv(nq, 256), 256, 0, s>>>(part_i, part_d, nq, slices, idx2, dist2, nq_count);
    } else {
        bf_knn2_kernel<false><<<dim3(qblocks, slices), 256, 0, s>>>(query, nq, (int)(qstride / 4), train, nt,
                                                                    (int)(tstride / 4), dim, slice_rows, part_i,
                                                                    part_d, vec_ok, nullptr, nullptr);
        MICV_LAUNCH_CHECK();
        bf_merge_kernel<false><<<cdiv(nq, 256), 256, 0, s>>>(part_i, part_d, nq, slices, idx2, dist2, nullptr);
    }
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

extern "C" {

int micv_bf_knn2_dev(micv_ctx *ctx, const float *query, int nq, size_t qstride, const float *train,
                     int nt, size_t tstride, int dim, int32_t *idx2, float *dist2,
                     micv_stream stream) {
    MICV_REQUIRE(ctx && query && train && idx2 && dist2, "micv_bf_knn2: null argument");
    MICV_REQUIRE(nq > 0 && nt >= 2 && dim > 0, "micv_bf_knn2: need nq > 0, nt >= 2, dim > 0");
    MICV_REQUIRE(stride_ok(qstride, dim, 4) && stride_ok(tstride, dim, 4), "micv_bf_knn2: bad stride");
    return bf_knn2_run(ctx, query, nq, qstride, nullptr, train, nt, tstride, nullptr, dim, idx2, dist2, stream);
}

int micv_bf_knn2_counted_dev(micv_ctx *ctx, const float *query, int nq_cap, size_t qstride, const int64_t *nq_count, const float *train,
                             int nt_cap, size_t tstride, const int64_t *nt_count, int dim, int32_t *idx2, float *dist2,
                             micv_stream stream) {
    MICV_REQUIRE(ctx && query && train && idx2 && dist2 && nq_count && nt_count, "micv_bf_knn2_counted: null argument");
    MICV_REQUIRE(nq_cap > 0 && nt_cap > 0 && dim > 0, "micv_bf_knn2_counted: need nq_cap > 0, nt_cap > 0, dim > 0");
    MICV_REQUIRE(stride_ok(qstride, dim, 4) && stride_ok(tstride, dim, 4), "micv_bf_knn2_counted: bad stride");
    return bf_knn2_run(ctx, query, nq_cap, qstride, nq_count, train, nt_cap, tstride, nt_count, dim, idx2, dist2, stream);
}

int micv_bf_match_pairs_dev(micv_ctx *ctx, const float *desc, int images, size_t dimage_stride, int cap, size_t dstride,
                            const int64_t *count, int dim, const int32_t *pairs, int npairs, double ratio, int32_t *idx2,
                            float *dist2, int32_t *matches_qt, float *distances, int64_t mcap, int64_t *match_count,
                            micv_stream stream) {
    MICV_REQUIRE(ctx && desc && pairs && match_count, "micv_bf_match_pairs: null argument");
    MICV_REQUIRE(!idx2 == !dist2, "micv_bf_match_pairs: idx2 and dist2 go together (both or neither)");
    MICV_REQUIRE(images >= 1 && cap >= 1 && dim >= 1, "micv_bf_match_pairs: need images >= 1, cap >= 1, dim >= 1");
    MICV_REQUIRE(npairs >= 1 && npairs <= 65535, "micv_bf_match_pairs: npairs %d outside 1 .. 65535", npairs);
    MICV_REQUIRE(mcap >= 0 && (mcap == 0 || (matches_qt && distances)), "micv_bf_match_pairs: bad mcap / outputs");
    MICV_REQUIRE(stride_ok(dstride, dim, 4), "micv_bf_match_pairs: bad stride");
    MICV_REQUIRE(dimage_stride % 4 == 0 && dimage_stride >= (size_t)(cap - 1) * dstride + (size_t)dim * 4,
                 "micv_bf_match_pairs: dimage_stride %zu is no multiple of 4 or below one image's rows", dimage_stride);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // S slices (the rule at bf_knn2_pairs_kernel), then as many pairs per launch as keep the partial lists in bound
    const int qblocks = (int)cdiv(cap, kQT), passes = (int)cdiv(cap, kTT);
    const size_t pair_bytes = (size_t)cap * sizeof(PairPart);  // one slice of one pair
    int64_t slices = std::min<int64_t>(((int64_t)kPairsWantWgs + (int64_t)qblocks * npairs - 1) / ((int64_t)qblocks * npairs), passes);
    slices = std::max<int64_t>(1, std::min<int64_t>(slices, (int64_t)(kPairsScratchBytes / pair_bytes)));
    const int piece = (int)std::max<size_t>(1, std::min<size_t>((size_t)npairs, kPairsScratchBytes / (pair_bytes * slices)));
    void *scratch;
    MICV_TRY(ctx->reserve((size_t)piece * slices * pair_bytes, &scratch));
    PairPart *part = static_cast<PairPart *>(scratch);
    const int vec_ok = ((reinterpret_cast<uintptr_t>(desc) | dstride | dimage_stride) & 15) == 0 && (dim & 3) == 0;
    for (int p0 = 0; p0 < npairs; p0 += piece) {  // (pieces reuse the partial lists: stream order keeps them apart)
        const int np = std::min(piece, npairs - p0);
        bf_knn2_pairs_kernel<<<dim3(qblocks, (unsigned)slices, np), 256, 0, s>>>(desc, images, dimage_stride / 4, cap, (int)(dstride / 4),
                                                                                 count, dim, pairs, p0, part, vec_ok);
        MICV_LAUNCH_CHECK();
        bf_finish_pairs_kernel<<<np, kFinishThreads, 0, s>>>(part, images, cap, count, pairs, p0, (int)slices, ratio, idx2,
                                                             dist2, matches_qt, distances, mcap, match_count);
        MICV_LAUNCH_CHECK();
    }
    return MICV_OK;
}

int micv_bf_ratio_filter_dev(micv_ctx *ctx, const int32_t *idx2, const float *dist2, int nq,
                             double ratio, int32_t *matches_qt, float *distances, int64_t cap,
                             int64_t *count, micv_stream stream) {
    MICV_REQUIRE(ctx && idx2 && dist2 && count, "micv_bf_ratio_filter: null argument");
    MICV_REQUIRE(nq > 0 && cap >= 0 && (cap == 0 || (matches_qt && distances)),
                 "micv_bf_ratio_filter: bad size / outputs");
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *scratch;
    MICV_TRY(ctx->reserve(Carver::need((size_t)cap + 1, 4) + compact_scratch_bytes(nq), &scratch));
    Carver c(scratch);
    int32_t *sel = c.take<int32_t>((size_t)cap + 1);
    MICV_TRY(ordered_compact(ctx, s, RatioPred{dist2, ratio}, IndexEmit{sel}, nq, cap, count, c.base + c.off));
    if (cap > 0) {
        bf_emit_kernel<<<64, 256, 0, s>>>(sel, count, cap, idx2, dist2, matches_qt, distances);
        MICV_LAUNCH_CHECK();
    }
    return MICV_OK;
}

}  // extern "C"
