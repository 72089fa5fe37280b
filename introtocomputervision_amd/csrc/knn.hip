// knn.hip -- ps7's classifier: cv::ml::KNearest (brute force, classifier mode) and matching::naiveConfusionMatrix /
// matching::confusionMatrix (ps7_cpp/lib/Matching.cpp).  The contract, written from OpenCV 3.4's knearest.cpp and
// marked unpinned there, is in include/mi_cv.h ("ps7: k-NN and confusion matrices").
//
//   knn_kernel<F64>        one lane per test row, 64 rows per workgroup: the train rows stream through LDS in tiles
//                          of 64, each lane keeps its k best (distance bits, response) in its own LDS column, then
//                          bubble-sorts the responses and takes the longest run.  A fold is a predicate on the train
//                          row (MODE_ALL: every row; MODE_LOO: not the test row itself; MODE_GROUPS: another group), so
//                          leave-one-out and leave-one-group-out over the same matrix are one launch each, with the
//                          train rows in their original order.
//   knn_confusion_kernel   one workgroup: integer counts in LDS (exact, so the order of the adds does not matter),
//                          then the f32 divisions and the average, as Matching.cpp does them.
#include <type_traits>

#include "common.hpp"

namespace micv {

namespace {

constexpr int kKnnLanes = 64, kKnnTile = 64;
enum { MODE_ALL = 0, MODE_LOO = 1, MODE_GROUPS = 2 };

__device__ __forceinline__ int dist_bits(float d) {
    // NaN compares above FLT_MAX whatever its sign bit (mi_cv.h): never inserted
    return d != d ? 0x7FC00000 : __builtin_bit_cast(int, d);
}

template <bool F64>
__device__ __forceinline__ float knn_dist(const float *u, const float *__restrict__ v, int dims) {
    // float: s += t0*t0 + t1*t1 + t2*t2 + t3*t3 per group of four, then single dims (knearest.cpp findNearestCore);
    // F64: the same with double s and double t = (double)(u - v) (CvKNearest::find_neighbors_direct, OpenCV 2.4)
    using T = typename std::conditional<F64, double, float>::type;
    T s = 0;
#pragma unroll
    for (int i = 0; i < MICV_KNN_MAX_DIMS; i += 4) {
        if (i + 4 <= dims) {
            const T t0 = (T)(u[i] - v[i]), t1 = (T)(u[i + 1] - v[i + 1]);
            const T t2 = (T)(u[i + 2] - v[i + 2]), t3 = (T)(u[i + 3] - v[i + 3]);
            s += t0 * t0 + t1 * t1 + t2 * t2 + t3 * t3;
        } else {
#pragma unroll
            for (int r = 0; r < 3; r++)
                if (i + r < dims) {
                    const T t0 = (T)(u[i + r] - v[i + r]);
                    s += t0 * t0;
                }
            break;
        }
    }
    return (float)s;
}

template <bool F64>
__global__ __launch_bounds__(kKnnLanes) void knn_kernel(const float *__restrict__ train, int ntrain, size_t tstride,
                                                         const int *__restrict__ tlabels, const int *__restrict__ tgroups,
                                                         const float *__restrict__ test, int ntest, size_t qstride,
                                                         int dims, int k, int mode, int ngroups, int *__restrict__ pred) {
    __shared__ float tile[kKnnTile * MICV_KNN_MAX_DIMS];
    __shared__ int tlab[kKnnTile], tgrp[kKnnTile];
    __shared__ int dd[MICV_KNN_MAX_K][kKnnLanes], nr[MICV_KNN_MAX_K][kKnnLanes];
    const int lane = threadIdx.x, row = blockIdx.x * kKnnLanes + lane;
    const int mygroup = (mode == MODE_GROUPS && row < ntest) ? tgroups[row] : 0;
    // a row whose group is outside 1..G is in no fold: never tested (its prediction is 0), always trained on
    const bool active = row < ntest && (mode != MODE_GROUPS || (mygroup >= 1 && mygroup <= ngroups));
    float u[MICV_KNN_MAX_DIMS];
#pragma unroll
    for (int i = 0; i < MICV_KNN_MAX_DIMS; i++) u[i] = (active && i < dims) ? test[(size_t)row * qstride + i] : 0.f;
    for (int i = 0; i < k; i++) {
        dd[i][lane] = 0x7F7FFFFF;  // FLT_MAX
        nr[i][lane] = 0;
    }
    int worst = 0x7F7FFFFF, eligible = 0;
    for (int j0 = 0; j0 < ntrain; j0 += kKnnTile) {
        const int nt = ntrain - j0 < kKnnTile ? ntrain - j0 : kKnnTile;
        __syncthreads();
        for (int e = lane; e < nt * dims; e += kKnnLanes) {
            const int r = e / dims, c = e - r * dims;
            tile[e] = train[(size_t)(j0 + r) * tstride + c];
        }
        if (lane < nt) {
            tlab[lane] = tlabels[j0 + lane];
            tgrp[lane] = mode == MODE_GROUPS ? tgroups[j0 + lane] : 0;
        }
        __syncthreads();
        if (!active) continue;
        for (int r = 0; r < nt; r++) {
            const int j = j0 + r;
            if (mode == MODE_LOO ? j == row : (mode == MODE_GROUPS && tgrp[r] == mygroup)) continue;
            eligible++;
            const int si = dist_bits(knn_dist<F64>(u, tile + r * dims, dims));
            if (si >= worst) continue;  // for (i = k; i > 0; i--) if (si >= dd[i-1]) break; if (i >= k) continue;
            int i = k - 1;
            while (i > 0 && si < dd[i - 1][lane]) {
                dd[i][lane] = dd[i - 1][lane];
                nr[i][lane] = nr[i - 1][lane];
                i--;
            }
            dd[i][lane] = si;
            nr[i][lane] = tlab[r];
            worst = dd[k - 1][lane];
        }
    }
    if (row >= ntest) return;
    if (!active) {
        pred[row] = 0;
        return;
    }
    // k = min(k, number of train rows): the first slots of the k-slot list are the shorter list
    const int ke = eligible < k ? eligible : k;
    int result = 0;
    if (ke > 0) {
        for (int j = ke - 1; j > 0; j--) {  // bubble sort, ascending
            bool sw = false;
            for (int i = 0; i < j; i++) {
                const int a = nr[i][lane], b = nr[i + 1][lane];
                if (a > b) {
                    nr[i][lane] = b;
                    nr[i + 1][lane] = a;
                    sw = true;
                }
            }
            if (!sw) break;
        }
        result = nr[0][lane];
        int prev = 0, best = 0;
        for (int j = 1; j <= ke; j++) {
            if (j == ke || nr[j][lane] != nr[j - 1][lane]) {
                const int count = j - prev;
                if (best < count) {
                    best = count;
                    result = nr[j - 1][lane];
                }
                prev = j;
            }
        }
    }
    pred[row] = result;
}

// mats: [G + 1 or 1][L][L] f32 (G per-group matrices then their average, or the one leave-one-out matrix).
__global__ __launch_bounds__(1024) void knn_confusion_kernel(const int *__restrict__ pred, const int *__restrict__ labels,
                                                              const int *__restrict__ groups, int n, int L, int G,
                                                              float *__restrict__ mats, int *__restrict__ left_out) {
    __shared__ int cnt[MICV_KNN_MAX_GROUPS][MICV_KNN_MAX_LABELS][MICV_KNN_MAX_LABELS];
    __shared__ int tot[MICV_KNN_MAX_GROUPS][MICV_KNN_MAX_LABELS];
    __shared__ int lost;
    const int nm = groups ? G : 1;
    for (int i = threadIdx.x; i < MICV_KNN_MAX_GROUPS * MICV_KNN_MAX_LABELS * MICV_KNN_MAX_LABELS; i += blockDim.x)
        (&cnt[0][0][0])[i] = 0;
    for (int i = threadIdx.x; i < MICV_KNN_MAX_GROUPS * MICV_KNN_MAX_LABELS; i += blockDim.x) (&tot[0][0])[i] = 0;
    if (threadIdx.x == 0) lost = 0;
    __syncthreads();
    int mylost = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int g = groups ? groups[i] : 1;
        if (g < 1 || g > nm) continue;  // in no fold: never tested
        const int e = labels[i], r = pred[i];
        if (e < 1 || e > L || r < 1 || r > L) {
            mylost++;
            continue;
        }
        __hip_atomic_fetch_add(&cnt[g - 1][e - 1][r - 1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&tot[g - 1][e - 1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (mylost) __hip_atomic_fetch_add(&lost, mylost, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    // counts of ones summed in f32 are these integers exactly (n < 2^24); cv::divide gives 0 where the count is 0
    for (int i = threadIdx.x; i < L * L; i += blockDim.x) {
        const int e = i / L, r = i % L;
        float avg = 0.f;
        for (int g = 0; g < nm; g++) {
            const float c = (float)cnt[g][e][r], t = (float)tot[g][e];
            const float v = t != 0.f ? c / t : 0.f;
            mats[((size_t)g * L + e) * L + r] = v;
            avg = avg + v;
        }
        if (groups) mats[((size_t)G * L + e) * L + r] = avg * (float)(1.0 / (double)G);  // convertTo(alpha = 1/G)
    }
    if (threadIdx.x == 0 && left_out) *left_out = lost;
}

}  // namespace

static int launch_knn(hipStream_t s, const float *train, int ntrain, size_t tstride, const int *tlabels,
                      const int *tgroups, const float *test, int ntest, size_t qstride, int dims, int k, int mode,
                      int ngroups, bool f64, int *pred) {
    const dim3 grid(cdiv(ntest, kKnnLanes));
    if (f64)
        knn_kernel<true><<<grid, kKnnLanes, 0, s>>>(train, ntrain, tstride, tlabels, tgroups, test, ntest, qstride, dims,
                                                   k, mode, ngroups, pred);
    else
        knn_kernel<false><<<grid, kKnnLanes, 0, s>>>(train, ntrain, tstride, tlabels, tgroups, test, ntest, qstride,
                                                    dims, k, mode, ngroups, pred);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // namespace micv

using namespace micv;

extern "C" {

int micv_knn_predict_dev(micv_ctx *ctx, const float *train, int ntrain, size_t train_stride, const int *train_labels,
                         const float *test, int ntest, size_t test_stride, int dims, int k, uint32_t flags, int *pred,
                         micv_stream stream) {
    MICV_REQUIRE(ctx && train && train_labels && test && pred, "micv_knn_predict: null argument");
    MICV_REQUIRE(ntrain >= 1 && ntest >= 1 && (uint64_t)ntrain < (1ull << 24) && (uint64_t)ntest < (1ull << 24),
                 "micv_knn_predict: row counts %d / %d outside 1 .. 2^24 - 1", ntrain, ntest);
    MICV_REQUIRE(dims >= 1 && dims <= MICV_KNN_MAX_DIMS, "micv_knn_predict: dims %d outside 1..%d", dims, MICV_KNN_MAX_DIMS);
    MICV_REQUIRE(k >= 1 && k <= MICV_KNN_MAX_K, "micv_knn_predict: k %d outside 1..%d", k, MICV_KNN_MAX_K);
    MICV_REQUIRE(stride_ok(train_stride, dims, 4) && stride_ok(test_stride, dims, 4), "micv_knn_predict: bad stride");
    MICV_REQUIRE((flags & ~(uint32_t)MICV_KNN_F64_ACC) == 0, "micv_knn_predict: unknown flags %#x", flags);
    MICV_HIP(hipSetDevice(ctx->device));
    return launch_knn(static_cast<hipStream_t>(stream), train, ntrain, train_stride / 4, train_labels, nullptr, test,
                      ntest, test_stride / 4, dims, k, MODE_ALL, 0, flags & MICV_KNN_F64_ACC, pred);
}

int micv_knn_confusion_dev(micv_ctx *ctx, const float *features, int n, size_t stride, int dims, const int *labels,
                           const int *groups, int num_labels, int num_groups, int k, uint32_t flags, float *confusion,
                           int *pred, int *left_out, micv_stream stream) {
    MICV_REQUIRE(ctx && features && labels && confusion, "micv_knn_confusion: null argument");
    MICV_REQUIRE(n >= 2 && (uint64_t)n < (1ull << 24), "micv_knn_confusion: %d rows outside 2 .. 2^24 - 1", n);
    MICV_REQUIRE(dims >= 1 && dims <= MICV_KNN_MAX_DIMS, "micv_knn_confusion: dims %d outside 1..%d", dims,
                 MICV_KNN_MAX_DIMS);
    MICV_REQUIRE(k >= 1 && k <= MICV_KNN_MAX_K, "micv_knn_confusion: k %d outside 1..%d", k, MICV_KNN_MAX_K);
    MICV_REQUIRE(stride_ok(stride, dims, 4), "micv_knn_confusion: bad stride");
    MICV_REQUIRE(num_labels >= 1 && num_labels <= MICV_KNN_MAX_LABELS, "micv_knn_confusion: %d labels outside 1..%d",
                 num_labels, MICV_KNN_MAX_LABELS);
    MICV_REQUIRE(!groups || (num_groups >= 1 && num_groups <= MICV_KNN_MAX_GROUPS),
                 "micv_knn_confusion: %d groups outside 1..%d", num_groups, MICV_KNN_MAX_GROUPS);
    MICV_REQUIRE((flags & ~(uint32_t)MICV_KNN_F64_ACC) == 0, "micv_knn_confusion: unknown flags %#x", flags);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int *p = pred;
    if (!p) {
        void *scratch;
        MICV_TRY(ctx->reserve(Carver::need((size_t)n, 4), &scratch));
        p = static_cast<int *>(scratch);
    }
    MICV_TRY(launch_knn(s, features, n, stride / 4, labels, groups, features, n, stride / 4, dims, k,
                        groups ? MODE_GROUPS : MODE_LOO, num_groups, flags & MICV_KNN_F64_ACC, p));
    knn_confusion_kernel<<<1, 1024, 0, s>>>(p, labels, groups, n, num_labels, groups ? num_groups : 1, confusion,
                                            left_out);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // extern "C"
