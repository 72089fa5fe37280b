// geom.hip -- ps3 on the device: camera calibration (normal equations and SVD), the fundamental
// matrix (normal equations, rank reduction, the normalised "extra credit" chain), epipolar end
// points and the camera centre (ps3_cpp/lib/{Calibration,Fundamental}.cpp, ps3_cpp/src/Solution.cpp),
// batched over T systems that share their point arrays and differ in an index list.
//
// One wave per system.  The small matrix lives in LDS (at most 11 x 12 words per wave) and one lane
// owns one matrix entry: it sums its entry over the rows in order, so a result depends neither on
// the grid nor on T.  The pivot search is the same short scan of the diagonal in every lane (first
// largest |d|), so there is no reduction whose order could vary.  Nothing is indexed at run time in
// a per-thread array (everything that pivoting permutes is in LDS).  The one-sided Jacobi keeps the
// columns of A in global scratch, lane l owning rows l, l + 64, ..., and V in LDS, lane i owning
// row i; its column sums are per-lane serial partials joined by an xor butterfly (32, 16, .., 1).
//
// Every kernel is a template on R, the arithmetic type: float (the reference's arithmetic) or double
// (MICV_GEOM_F64: the same operations in the same order, inputs still f32, outputs rounded once).
// The contract is in include/mi_cv.h ("ps3: geometry") and DESIGN.md section 2.  -ffp-contract=off:
// no fused multiply-add anywhere here.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <numeric>
#include <random>
#include <vector>

#include "common.hpp"
#include "epipolar.hpp"

struct micv_ransac_rng {  // ransac.hip
    std::mt19937 eng;
};

namespace micv {
namespace {

constexpr int kWaves = 4;          // 256-thread workgroups, one system per wave at a time
constexpr int kStageMax = 2048;    // points staged in LDS (20 B each)
constexpr int kMaxTests = 64;      // test points per trial: one lane each
constexpr int kMaxSweeps = 30;     // Jacobi sweep cap
constexpr int kMaxGroups = 64;
constexpr int kSvdMaxK = 1024;

struct Groups {
    int off[kMaxGroups + 1];
    int G;
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ inline float absr(float v) { return fabsf(v); }
__device__ inline double absr(double v) { return fabs(v); }
__device__ inline float sqrtr(float v) { return sqrtf(v); }
__device__ inline double sqrtr(double v) { return sqrt(v); }

template <typename R>
__device__ inline R nan_of();
template <>
__device__ inline float nan_of<float>() { return __int_as_float(0x7FC00000); }
template <>
__device__ inline double nan_of<double>() { return __longlong_as_double(0x7FF8000000000000ll); }

__device__ inline uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <typename R>
__device__ inline R butterfly(R v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// Diagonal-pivoted LDL^T of the symmetric N x N matrix in S (row-major, N + 1 columns: the last
// one is the right-hand side) and the solve, x[N] in LDS.  Step p: the pivot is the first largest
// |S[i][i]|, i >= p (a NaN is never larger); rows and columns p, q are swapped; every entry (i, j),
// i, j > p, becomes S[i][j] - (S[p][max(i,j)] / d) * S[p][min(i,j)], the right-hand side
// b[i] - (S[p][i] / d) * b[p]; column p keeps L[i][p] = S[p][i] / d.  Then z[p] = b[p] / d[p] and
// x[p] = z[p] - L[p+1][p] x[p+1] - ... - L[N-1][p] x[N-1] (ascending), p descending, and the
// transpositions undone in reverse.  A zero pivot divides by zero: inf / NaN come out.
template <typename R, int N>
__device__ inline void ldlt_solve(R *S, R *x, int *perm, int lane) {
    constexpr int W = N + 1;
    for (int p = 0; p < N; p++) {
        int q = p;
        R best = absr(S[p * W + p]);
        for (int i = p + 1; i < N; i++) {
            const R v = absr(S[i * W + i]);
            if (v > best) {
                best = v;
                q = i;
            }
        }
        if (q != p) {
            if (lane < W) {
                const R a = S[p * W + lane], b = S[q * W + lane];
                S[p * W + lane] = b;
                S[q * W + lane] = a;
            }
            wave_sync();
            if (lane < N) {
                const R a = S[lane * W + p], b = S[lane * W + q];
                S[lane * W + p] = b;
                S[lane * W + q] = a;
            }
            wave_sync();
        }
        if (lane == 0) perm[p] = q;
        const R d = S[p * W + p];
        const int m = N - 1 - p;
        const int cnt = m * (m + 1);
        for (int e = lane; e < cnt; e += 64) {
            const int i = p + 1 + e / (m + 1), jj = p + 1 + e % (m + 1);
            const int hi = jj < N ? (i > jj ? i : jj) : i;
            const int lo = jj < N ? (i > jj ? jj : i) : N;
            const R l = S[p * W + hi] / d;
            S[i * W + jj] = S[i * W + jj] - l * S[p * W + lo];
        }
        if (lane > p && lane < N) S[lane * W + p] = S[p * W + lane] / d;
        wave_sync();
    }
    if (lane == 0) {
        for (int p = N - 1; p >= 0; p--) {
            R s = S[p * W + N] / S[p * W + p];
            for (int i = p + 1; i < N; i++) s = s - S[i * W + p] * x[i];
            x[p] = s;
        }
        for (int p = N - 1; p >= 0; p--) {
            const int q = perm[p];
            const R a = x[p], b = x[q];
            x[p] = b;
            x[q] = a;
        }
    }
    wave_sync();
}

// Entry c of row `row` (0: the x row, 1: the y row) of the calibration system of one point;
// u is x or y.  c = 11 is the right-hand side (normal equations) or -u (SVD, `svd`).
template <typename R>
__device__ inline R calib_elem(int row, int c, R X, R Y, R Z, R u, bool svd) {
    if (c < 8) {
        const int cc = c - 4 * row;
        if (cc < 0 || cc > 3) return (R)0;
        return cc == 0 ? X : cc == 1 ? Y : cc == 2 ? Z : (R)1;
    }
    if (c == 11) return svd ? -u : u;
    return (-u) * (c == 8 ? X : c == 9 ? Y : Z);
}

template <typename R, typename P>
__device__ inline R fund_elem(int c, P ua, P va, P ub, P vb) {
    const R u = (R)ua, v = (R)va, up = (R)ub, vp = (R)vb;
    switch (c) {
    case 0: return u * up;
    case 1: return v * up;
    case 2: return up;
    case 3: return u * vp;
    case 4: return v * vp;
    case 5: return vp;
    case 6: return u;
    case 7: return v;
    default: return (R)-1;
    }
}

// calib::solveLeastSquares for T index subsets + the trial residual of Solution.cpp:243-318.
template <typename R>
__global__ __launch_bounds__(256) void calib_ls_kernel(const float *__restrict__ pts2d, const float *__restrict__ pts3d,
                                                       int n, int staged, const int32_t *__restrict__ indices,
                                                       int stride, const int32_t *__restrict__ kcount, int k, int j,
                                                       int T, float *__restrict__ M, double *__restrict__ residual,
                                                       int32_t *status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ R Sall[kWaves][11 * 12];
    __shared__ R xall[kWaves][12];
    __shared__ int pall[kWaves][12];
    __shared__ double nall[kWaves][kMaxTests];
    const float *p2 = pts2d, *p3 = pts3d;
    if (staged) {
        float *l3 = reinterpret_cast<float *>(smem), *l2 = l3 + 3 * (size_t)n;
        for (int i = threadIdx.x; i < 3 * n; i += blockDim.x) l3[i] = pts3d[i];
        for (int i = threadIdx.x; i < 2 * n; i += blockDim.x) l2[i] = pts2d[i];
        __syncthreads();
        p3 = l3;
        p2 = l2;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    R *S = Sall[wave], *x = xall[wave];
    int *perm = pall[wave];
    double *nrm = nall[wave];
    for (int64_t t = (int64_t)blockIdx.x * kWaves + wave; t < T; t += (int64_t)gridDim.x * kWaves) {
        const int32_t *idx = indices ? indices + (size_t)t * stride : nullptr;
        const int kc = kcount ? kcount[t] : k;
        bool ok = kc >= 0 && kc <= k;
        if (ok && idx)
            for (int i = lane; i < kc + j; i += 64) ok = ok && idx[i] >= 0 && idx[i] < n;
        if (__any(!ok)) {
            if (lane == 0) {
                atomicOr(status, 1);
                residual[t] = nan_of<double>();
            }
            if (lane < 12) M[(size_t)t * 12 + lane] = nan_of<float>();
            continue;
        }
        for (int e = lane; e < 11 * 12; e += 64) {
            const int r = e / 12, c = e % 12;
            R s = (R)0;
            for (int i = 0; i < kc; i++) {
                const int id = idx ? idx[i] : i;
                const R X = (R)p3[3 * id], Y = (R)p3[3 * id + 1], Z = (R)p3[3 * id + 2];
                const R px = (R)p2[2 * id], py = (R)p2[2 * id + 1];
                s = s + calib_elem<R>(0, r, X, Y, Z, px, false) * calib_elem<R>(0, c, X, Y, Z, px, false);
                s = s + calib_elem<R>(1, r, X, Y, Z, py, false) * calib_elem<R>(1, c, X, Y, Z, py, false);
            }
            S[e] = s;
        }
        wave_sync();
        ldlt_solve<R, 11>(S, x, perm, lane);
        if (lane == 11) x[11] = (R)1;
        wave_sync();
        if (lane < 12) M[(size_t)t * 12 + lane] = (float)x[lane];
        if (lane < j) {
            const int id = idx ? idx[kc + lane] : kc + lane;
            const double X = p3[3 * id], Y = p3[3 * id + 1], Z = p3[3 * id + 2];
            R pr[3];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                double s = (double)x[4 * r] * X;
                s = s + (double)x[4 * r + 1] * Y;
                s = s + (double)x[4 * r + 2] * Z;
                s = s + (double)x[4 * r + 3] * 1.0;
                pr[r] = (R)s;
            }
            const R rc = (R)(1.0 / (double)pr[2]);
            const double d0 = (double)(pr[0] * rc - (R)p2[2 * id]);
            const double d1 = (double)(pr[1] * rc - (R)p2[2 * id + 1]);
            nrm[lane] = sqrt(d0 * d0 + d1 * d1);
        }
        wave_sync();
        if (lane == 0) {
            double s = 0.0;
            for (int i = 0; i < j; i++) s = s + nrm[i];
            residual[t] = s / (double)j;
        }
        wave_sync();
    }
}

// First strict minimum of the residuals of each group (blocks 0 .. G-1) and of all trials (block G).
__global__ __launch_bounds__(256) void geom_argmin_kernel(const double *__restrict__ residual,
                                                          const float *__restrict__ M, Groups g, int T,
                                                          int32_t *best_idx, double *best_res, float *best_M) {
    __shared__ double sr[256];
    __shared__ int si[256];
    const int b = blockIdx.x;
    const int lo = b < g.G ? g.off[b] : 0, hi = b < g.G ? g.off[b + 1] : T;
    double br = DBL_MAX;
    int bi = INT_MAX;
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        const double r = residual[i];
        if (r < br) {
            br = r;
            bi = i;
        }
    }
    sr[threadIdx.x] = br;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const double r = sr[threadIdx.x + w];
            const int i = si[threadIdx.x + w];
            if (r < sr[threadIdx.x] || (r == sr[threadIdx.x] && i < si[threadIdx.x])) {
                sr[threadIdx.x] = r;
                si[threadIdx.x] = i;
            }
        }
        __syncthreads();
    }
    const int win = si[0];
    if (threadIdx.x == 0) {
        best_idx[b] = win == INT_MAX ? -1 : win;
        best_res[b] = sr[0];
    }
    if (threadIdx.x < 12) best_M[(size_t)b * 12 + threadIdx.x] = win == INT_MAX ? 0.f : M[(size_t)win * 12 + threadIdx.x];
}

// fundamental::solveLeastSquares for T index subsets (indices NULL: the points 0 .. k-1).
template <typename R, typename P>
__global__ __launch_bounds__(256) void fund_ls_kernel(const P *__restrict__ ptsA, const P *__restrict__ ptsB, int n,
                                                      const int32_t *__restrict__ indices, int stride, int k, int T,
                                                      float *__restrict__ F, R *__restrict__ raw, int32_t *status) {
    __shared__ R Sall[kWaves][8 * 9];
    __shared__ R xall[kWaves][8];
    __shared__ int pall[kWaves][8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    R *S = Sall[wave], *x = xall[wave];
    int *perm = pall[wave];
    for (int64_t t = (int64_t)blockIdx.x * kWaves + wave; t < T; t += (int64_t)gridDim.x * kWaves) {
        const int32_t *idx = indices ? indices + (size_t)t * stride : nullptr;
        bool ok = true;
        if (idx)
            for (int i = lane; i < k; i += 64) ok = ok && idx[i] >= 0 && idx[i] < n;
        if (__any(!ok)) {
            if (lane == 0) atomicOr(status, 1);
            if (lane < 9) {
                if (F) F[(size_t)t * 9 + lane] = nan_of<float>();
                if (raw) raw[(size_t)t * 9 + lane] = nan_of<R>();
            }
            continue;
        }
        for (int e = lane; e < 8 * 9; e += 64) {
            const int r = e / 9, c = e % 9;
            R s = (R)0;
            for (int i = 0; i < k; i++) {
                const int id = idx ? idx[i] : i;
                const P ua = ptsA[2 * id], va = ptsA[2 * id + 1], ub = ptsB[2 * id], vb = ptsB[2 * id + 1];
                s = s + fund_elem<R, P>(r, ua, va, ub, vb) * fund_elem<R, P>(c, ua, va, ub, vb);
            }
            S[e] = s;
        }
        wave_sync();
        ldlt_solve<R, 8>(S, x, perm, lane);
        if (lane < 9) {
            const R v = lane < 8 ? x[lane] : (R)1;
            if (F) F[(size_t)t * 9 + lane] = (float)v;
            if (raw) raw[(size_t)t * 9 + lane] = v;
        }
        wave_sync();
    }
}

// One-sided (Hestenes) Jacobi on the NC columns of a rows x NC matrix, one wave per system.
//   MODE 0: the 2k x 12 system of calib::solveSVD; out = the column of V of the smallest column norm.
//   MODE 1: a 3 x 3 matrix (row-major, type P); out = fundamental::rankReduce.
// Pairs (p, q), p < q, in cyclic order (0,1), (0,2), .., (NC-2,NC-1).  alpha = S a_p^2, beta = S a_q^2,
// gamma = S a_p a_q, each lane summing its rows l, l + 64, .. in order from 0 and the 64 partials
// joined by v = v + shfl_xor(v, m), m = 32, 16, .., 1.  The pair rotates when
// |gamma| > eps * sqrt(alpha * beta) (eps 1e-7 in float, 1e-15 in double):
//   zeta = (beta - alpha) / (2 gamma), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (sign(0) = +1),
//   c = 1 / sqrt(1 + t^2), s = c t, a_p' = c a_p - s a_q, a_q' = s a_p + c a_q, and the same on V.
// A sweep without a rotation, or kMaxSweeps sweeps, end the loop.
template <typename R, typename P, int NC, int MODE>
__global__ __launch_bounds__(256) void jacobi_kernel(const float *__restrict__ pts2d, const float *__restrict__ pts3d,
                                                     int n, const int32_t *__restrict__ indices, int stride, int k,
                                                     const P *__restrict__ mats, int T, R *__restrict__ work,
                                                     float *__restrict__ out, R *__restrict__ raw, int32_t *status) {
    __shared__ R Vall[kWaves][NC * NC];
    __shared__ R nall[kWaves][NC];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    R *V = Vall[wave], *cn = nall[wave];
    const int rows = MODE == 0 ? 2 * k : 3;
    const R eps = sizeof(R) == 4 ? (R)1e-7f : (R)1e-15;
    for (int64_t t = (int64_t)blockIdx.x * kWaves + wave; t < T; t += (int64_t)gridDim.x * kWaves) {
        R *A = work + (size_t)t * NC * rows;  // column-major: A[c * rows + r]
        if (MODE == 0) {
            const int32_t *idx = indices ? indices + (size_t)t * stride : nullptr;
            bool ok = true;
            if (idx)
                for (int i = lane; i < k; i += 64) ok = ok && idx[i] >= 0 && idx[i] < n;
            if (__any(!ok)) {
                if (lane == 0) atomicOr(status, 1);
                if (lane < 12) out[(size_t)t * 12 + lane] = nan_of<float>();
                continue;
            }
            for (int r = lane; r < rows; r += 64) {
                const int i = r >> 1, row = r & 1;
                const int id = idx ? idx[i] : i;
                const R X = (R)pts3d[3 * id], Y = (R)pts3d[3 * id + 1], Z = (R)pts3d[3 * id + 2];
                const R u = (R)pts2d[2 * id + row];
                for (int c = 0; c < NC; c++) A[c * rows + r] = calib_elem<R>(row, c, X, Y, Z, u, true);
            }
        } else {
            if (lane < 3)
                for (int c = 0; c < NC; c++) A[c * rows + lane] = (R)mats[(size_t)t * 9 + lane * 3 + c];
        }
        if (lane < NC)
            for (int c = 0; c < NC; c++) V[lane * NC + c] = lane == c ? (R)1 : (R)0;
        for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
            int rot = 0;
            for (int p = 0; p < NC - 1; p++)
                for (int q = p + 1; q < NC; q++) {
                    R al = (R)0, be = (R)0, ga = (R)0;
                    for (int r = lane; r < rows; r += 64) {
                        const R ap = A[p * rows + r], aq = A[q * rows + r];
                        al = al + ap * ap;
                        be = be + aq * aq;
                        ga = ga + ap * aq;
                    }
                    al = butterfly(al);
                    be = butterfly(be);
                    ga = butterfly(ga);
                    if (!(absr(ga) > eps * sqrtr(al * be))) continue;
                    rot++;
                    const R zeta = (be - al) / ((R)2 * ga);
                    const R tt = (zeta >= (R)0 ? (R)1 : (R)-1) / (absr(zeta) + sqrtr((R)1 + zeta * zeta));
                    const R cs = (R)1 / sqrtr((R)1 + tt * tt);
                    const R sn = cs * tt;
                    for (int r = lane; r < rows; r += 64) {
                        const R ap = A[p * rows + r], aq = A[q * rows + r];
                        A[p * rows + r] = cs * ap - sn * aq;
                        A[q * rows + r] = sn * ap + cs * aq;
                    }
                    if (lane < NC) {
                        const R vp = V[lane * NC + p], vq = V[lane * NC + q];
                        V[lane * NC + p] = cs * vp - sn * vq;
                        V[lane * NC + q] = sn * vp + cs * vq;
                    }
                }
            if (rot == 0) break;
        }
        for (int c = 0; c < NC; c++) {
            R s = (R)0;
            for (int r = lane; r < rows; r += 64) {
                const R a = A[c * rows + r];
                s = s + a * a;
            }
            s = butterfly(s);
            if (lane == 0) cn[c] = s;
        }
        wave_sync();
        int m = 0;
        for (int c = 1; c < NC; c++)
            if (cn[c] < cn[m]) m = c;
        if (MODE == 0) {
            if (lane < NC) {
                const R v = V[lane * NC + m];
                out[(size_t)t * NC + lane] = (float)v;
            }
        } else {
            // U Sigma V^T with the smallest singular value zeroed: column m of the rotated A is 0
            __shared__ R Aall[kWaves][9];
            R *As = Aall[wave];
            if (lane < 3)
                for (int c = 0; c < 3; c++) As[c * 3 + lane] = c == m ? (R)0 : A[c * rows + lane];
            wave_sync();
            if (lane < 9) {
                const int r = lane / 3, c = lane % 3;
                R s = (R)0;
                for (int jn = 0; jn < 3; jn++) s = s + As[jn * 3 + r] * V[c * 3 + jn];
                if (out) out[(size_t)t * 9 + lane] = (float)s;
                if (raw) raw[(size_t)t * 9 + lane] = s;
            }
        }
        wave_sync();
    }
}

// C = A B for 3 x 3: double accumulation from the first product, ascending, one rounding to R
// (the gemm rule of DESIGN.md section 2, "RANSAC").
template <typename R>
__device__ inline void gemm3(const R *A, const R *B, R *C) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double s = (double)A[r * 3] * (double)B[c];
            s = s + (double)A[r * 3 + 1] * (double)B[3 + c];
            s = s + (double)A[r * 3 + 2] * (double)B[6 + c];
            C[r * 3 + c] = (R)s;
        }
}

// Solution.cpp:381-445 up to the normalised points: T = scale * offset per image and T * [x y 1].
template <typename R>
__global__ __launch_bounds__(256) void fnorm_prep_kernel(const float *__restrict__ ptsA, const float *__restrict__ ptsB,
                                                         int n, R *__restrict__ Tab, R *__restrict__ nA,
                                                         R *__restrict__ nB) {
    __shared__ R Ts[18];
    if (threadIdx.x < 2) {
        const float *p = threadIdx.x ? ptsB : ptsA;
        R mean[2];
        for (int d = 0; d < 2; d++) {
            // cv::mean: a double chain over partial sums of four
            double s = 0.0;
            int i = 0;
            for (; i + 4 <= n; i += 4)
                s = s + (double)((((R)p[2 * i + d] + (R)p[2 * i + 2 + d]) + (R)p[2 * i + 4 + d]) + (R)p[2 * i + 6 + d]);
            for (; i < n; i++) s = s + (double)(R)p[2 * i + d];
            mean[d] = (R)(s / (double)n);
        }
        R mx = (R)1;  // the appended row of ones takes part in the maximum
        for (int i = 0; i < 2 * n; i++) {
            const R v = absr((R)p[i]);
            if (v > mx) mx = v;
        }
        const R sc = (R)(1.0 / (double)mx);
        const R scale[9] = {sc, 0, 0, 0, sc, 0, 0, 0, 1};
        const R offset[9] = {1, 0, -mean[0], 0, 1, -mean[1], 0, 0, 1};
        R Tm[9];
        gemm3<R>(scale, offset, Tm);
        for (int e = 0; e < 9; e++) {
            Ts[threadIdx.x * 9 + e] = Tm[e];
            Tab[threadIdx.x * 9 + e] = Tm[e];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * n; i += blockDim.x) {
        const int pt = i >> 1, d = i & 1;
        for (int w = 0; w < 2; w++) {
            const float *p = w ? ptsB : ptsA;
            const R *Tm = Ts + 9 * w;
            double s = (double)Tm[3 * d] * (double)p[2 * pt];
            s = s + (double)Tm[3 * d + 1] * (double)p[2 * pt + 1];
            s = s + (double)Tm[3 * d + 2] * 1.0;
            (w ? nB : nA)[i] = (R)s;
        }
    }
}

// F = T_b^T F_Hat T_a, (T_b^T F_Hat) first, and the four outputs as f32.
template <typename R>
__global__ void fnorm_compose_kernel(const R *__restrict__ Tab, const R *__restrict__ Fhat, float *Ta, float *Tb,
                                     float *Fh, float *F) {
    if (threadIdx.x || blockIdx.x) return;
    R TbT[9], t1[9], t2[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) TbT[r * 3 + c] = Tab[9 + c * 3 + r];
    gemm3<R>(TbT, Fhat, t1);
    gemm3<R>(t1, Tab, t2);
    for (int e = 0; e < 9; e++) {
        Ta[e] = (float)Tab[e];
        Tb[e] = (float)Tab[9 + e];
        Fh[e] = (float)Fhat[e];
        F[e] = (float)t2[e];
    }
}

// Solution.cpp:343-362 and :124-163: the epipolar line of each point and its intersections with
// the left and right image borders, each scaled by the reciprocal of its third coordinate (epipolar.hpp).
template <typename R>
__global__ __launch_bounds__(256) void epipolar_kernel(const float *__restrict__ F, const float *__restrict__ pts, int n,
                                                       int side, int rows, int cols, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float e[6];
    epipolar_endpoints<R>(F, pts[2 * (size_t)i], pts[2 * (size_t)i + 1], side, rows, cols, e);
    for (int c = 0; c < 6; c++) out[6 * (size_t)i + c] = e[c];
}

// Solution.cpp:320-326: -Q^-1 m4.  Q^-1 is the closed form ransac.hip restates for a 3 x 3 CV_32F
// cv::invert: determinant and cofactors in double, each rounded once (zeros when det == 0).
template <typename R>
__global__ __launch_bounds__(256) void camera_center_kernel(const float *__restrict__ M, int T, float *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const float *m = M + 12 * (size_t)t;
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    R I[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (det != 0.) {
        det = 1. / det;
        I[0] = (R)((e * i - f * h) * det);
        I[1] = (R)((c * h - b * i) * det);
        I[2] = (R)((b * f - c * e) * det);
        I[3] = (R)((f * g - d * i) * det);
        I[4] = (R)((a * i - c * g) * det);
        I[5] = (R)((c * d - a * f) * det);
        I[6] = (R)((d * h - e * g) * det);
        I[7] = (R)((b * g - a * h) * det);
        I[8] = (R)((a * e - b * d) * det);
    }
    for (int r = 0; r < 3; r++) {
        double s = (double)I[3 * r] * (double)m[3];
        s = s + (double)I[3 * r + 1] * (double)m[7];
        s = s + (double)I[3 * r + 2] * (double)m[11];
        out[3 * (size_t)t + r] = (float)(R)(-1.0 * s);
    }
}

// The counter-based sampler of mi_cv.h: `count` distinct indices of [0, n) per trial.
__global__ __launch_bounds__(256) void geom_sample_kernel(uint64_t seed, int n, int count, int64_t T,
                                                          int32_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    int32_t *o = out + (size_t)t * count;
    for (int e = 0; e < count; e++) {
        for (uint32_t a = 0;; a++) {
            const uint64_t r = splitmix64(seed ^ (((uint64_t)(uint32_t)t << 32) | ((uint64_t)e << 20) | (a & 0xFFFFFu)));
            const int idx = (int)(((r >> 32) * (uint64_t)(uint32_t)n) >> 32);
            bool dup = false;
            for (int q = 0; q < e; q++) dup |= o[q] == idx;
            if (!dup) {
                o[e] = idx;
                break;
            }
        }
    }
}

int grid_for(micv_ctx *ctx, int64_t T) {
    const int64_t blocks = (T + kWaves - 1) / kWaves;
    return (int)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)ctx->wave_slots(2) / kWaves));
}

template <typename R>
int calib_ls_launch(micv_ctx *ctx, hipStream_t s, const float *pts2d, const float *pts3d, int n, const int32_t *indices,
                    int stride, const int32_t *kcount, int k, int j, int T, float *M, double *residual,
                    int32_t *status) {
    const int staged = n <= kStageMax;
    calib_ls_kernel<R><<<grid_for(ctx, T), 64 * kWaves, staged ? (size_t)n * 20 : 0, s>>>(
        pts2d, pts3d, n, staged, indices, stride, kcount, k, j, T, M, residual, status);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

template <typename R>
int svd_launch(micv_ctx *ctx, hipStream_t s, const float *pts2d, const float *pts3d, int n, const int32_t *indices,
               int stride, int k, int T, float *M, int32_t *status) {
    void *scratch;
    MICV_TRY(ctx->reserve(Carver::need((size_t)T * 24 * (size_t)k, sizeof(R)), &scratch));
    jacobi_kernel<R, float, 12, 0><<<grid_for(ctx, T), 64 * kWaves, 0, s>>>(
        pts2d, pts3d, n, indices, stride, k, nullptr, T, static_cast<R *>(scratch), M, nullptr, status);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

template <typename R>
int rank_launch(micv_ctx *ctx, hipStream_t s, const float *F, int T, float *out) {
    void *scratch;
    MICV_TRY(ctx->reserve(Carver::need((size_t)T * 9, sizeof(R)), &scratch));
    jacobi_kernel<R, float, 3, 1><<<grid_for(ctx, T), 64 * kWaves, 0, s>>>(nullptr, nullptr, 0, nullptr, 0, 0, F, T,
                                                                          static_cast<R *>(scratch), out, nullptr,
                                                                          nullptr);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

template <typename R>
int normalized_launch(micv_ctx *ctx, hipStream_t s, const float *ptsA, const float *ptsB, int n, float *Ta, float *Tb,
                      float *Fh, float *F) {
    void *scratch;
    MICV_TRY(ctx->reserve(4 * Carver::need(18, sizeof(R)) + 2 * Carver::need(2 * (size_t)n, sizeof(R)), &scratch));
    Carver c(scratch);
    R *Tab = c.take<R>(18), *est = c.take<R>(18), *fhat = c.take<R>(18), *work = c.take<R>(18);
    R *nA = c.take<R>(2 * (size_t)n), *nB = c.take<R>(2 * (size_t)n);
    fnorm_prep_kernel<R><<<1, 256, 0, s>>>(ptsA, ptsB, n, Tab, nA, nB);
    MICV_LAUNCH_CHECK();
    fund_ls_kernel<R, R><<<1, 64 * kWaves, 0, s>>>(nA, nB, n, nullptr, 0, n, 1, nullptr, est, nullptr);
    MICV_LAUNCH_CHECK();
    jacobi_kernel<R, R, 3, 1><<<1, 64 * kWaves, 0, s>>>(nullptr, nullptr, 0, nullptr, 0, 0, est, 1, work, nullptr, fhat,
                                                       nullptr);
    MICV_LAUNCH_CHECK();
    fnorm_compose_kernel<R><<<1, 64, 0, s>>>(Tab, fhat, Ta, Tb, Fh, F);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // namespace
}  // namespace micv

using namespace micv;

extern "C" {

int micv_geom_trial_indices(micv_ransac_rng *rng, int64_t n, int trials, int32_t *out) {
    MICV_REQUIRE(rng && out && n >= 1 && n <= (int64_t)1 << 30 && trials >= 0, "micv_geom_trial_indices: bad argument");
    std::vector<int> idx((size_t)n);
    for (int t = 0; t < trials; t++) {
        std::iota(idx.begin(), idx.end(), 0);
        std::shuffle(idx.begin(), idx.end(), rng->eng);
        std::copy(idx.begin(), idx.end(), out + (size_t)t * (size_t)n);
    }
    return MICV_OK;
}

int micv_geom_sample_indices_dev(micv_ctx *ctx, uint64_t seed, int n, int count, int64_t T, int32_t *out,
                                 micv_stream stream) {
    MICV_REQUIRE(ctx && out, "micv_geom_sample_indices_dev: null argument");
    MICV_REQUIRE(n >= 1 && count >= 1 && count <= n && count <= 4096 && T >= 1 && T <= 0x7FFFFFFF,
                 "micv_geom_sample_indices_dev: need 1 <= count <= min(n, 4096) and 1 <= T < 2^31 (n %d, count %d)", n,
                 count);
    MICV_HIP(hipSetDevice(ctx->device));
    geom_sample_kernel<<<(unsigned)((T + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(seed, n, count, T, out);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_calib_ls_trials_dev(micv_ctx *ctx, const float *pts2d, const float *pts3d, int n, const int32_t *indices,
                             int stride, int k, int j, int T, const int32_t *kcount, const int *group_sizes, int G,
                             uint32_t flags, float *M, double *residual, int32_t *best_idx, double *best_res,
                             float *best_M, int32_t *status, micv_stream stream) {
    MICV_REQUIRE(ctx && pts2d && pts3d && M && residual && status, "micv_calib_ls_trials_dev: null argument");
    MICV_REQUIRE((best_idx != nullptr) == (best_res != nullptr) && (best_idx != nullptr) == (best_M != nullptr),
                 "micv_calib_ls_trials_dev: best_idx, best_res and best_M go together");
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64), "micv_calib_ls_trials_dev: unknown flags %u", flags);
    MICV_REQUIRE(n >= 1 && n <= 1 << 24 && k >= 0 && j >= 0 && j <= kMaxTests && (int64_t)k + j <= n && T >= 1,
                 "micv_calib_ls_trials_dev: need 1 <= n <= 2^24, k >= 0, 0 <= j <= 64, k + j <= n, T >= 1 (n %d, k %d, "
                 "j %d, T %d)", n, k, j, T);
    MICV_REQUIRE(indices ? stride >= k + j : (T == 1 && !kcount),
                 "micv_calib_ls_trials_dev: stride %d < k + j, or no indices with T != 1", stride);
    Groups g;
    g.G = 0;
    g.off[0] = 0;
    if (group_sizes) {
        MICV_REQUIRE(best_idx && G >= 1 && G <= kMaxGroups, "micv_calib_ls_trials_dev: 1 <= G <= %d groups need the "
                     "arg-min outputs", kMaxGroups);
        int64_t sum = 0;
        for (int i = 0; i < G; i++) {
            MICV_REQUIRE(group_sizes[i] >= 0, "micv_calib_ls_trials_dev: negative group size");
            sum += group_sizes[i];
            g.off[i + 1] = (int)std::min<int64_t>(sum, T);
        }
        MICV_REQUIRE(sum == T, "micv_calib_ls_trials_dev: group sizes sum to %lld, not T = %d", (long long)sum, T);
        g.G = G;
    } else {
        MICV_REQUIRE(G == 0, "micv_calib_ls_trials_dev: G = %d without group_sizes", G);
    }
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    MICV_HIP(hipMemsetAsync(status, 0, 4, s));
    if (flags & MICV_GEOM_F64)
        MICV_TRY(calib_ls_launch<double>(ctx, s, pts2d, pts3d, n, indices, stride, kcount, k, j, T, M, residual, status));
    else
        MICV_TRY(calib_ls_launch<float>(ctx, s, pts2d, pts3d, n, indices, stride, kcount, k, j, T, M, residual, status));
    if (best_idx) {
        geom_argmin_kernel<<<g.G + 1, 256, 0, s>>>(residual, M, g, T, best_idx, best_res, best_M);
        MICV_LAUNCH_CHECK();
    }
    return MICV_OK;
}

int micv_calib_svd_dev(micv_ctx *ctx, const float *pts2d, const float *pts3d, int n, const int32_t *indices, int stride,
                       int k, int T, uint32_t flags, float *M, int32_t *status, micv_stream stream) {
    MICV_REQUIRE(ctx && pts2d && pts3d && M && status, "micv_calib_svd_dev: null argument");
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64), "micv_calib_svd_dev: unknown flags %u", flags);
    MICV_REQUIRE(n >= 1 && n <= 1 << 24 && k >= 1 && k <= kSvdMaxK && k <= n && T >= 1 &&
                     (indices ? stride >= k : T == 1),
                 "micv_calib_svd_dev: need 1 <= k <= min(n, %d), T >= 1, stride >= k (n %d, k %d, T %d, stride %d)",
                 kSvdMaxK, n, k, T, stride);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    MICV_HIP(hipMemsetAsync(status, 0, 4, s));
    if (flags & MICV_GEOM_F64) return svd_launch<double>(ctx, s, pts2d, pts3d, n, indices, stride, k, T, M, status);
    return svd_launch<float>(ctx, s, pts2d, pts3d, n, indices, stride, k, T, M, status);
}

int micv_fundamental_ls_dev(micv_ctx *ctx, const float *ptsA, const float *ptsB, int n, const int32_t *indices,
                            int stride, int k, int T, uint32_t flags, float *F, int32_t *status, micv_stream stream) {
    MICV_REQUIRE(ctx && ptsA && ptsB && F && status, "micv_fundamental_ls_dev: null argument");
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64), "micv_fundamental_ls_dev: unknown flags %u", flags);
    MICV_REQUIRE(n >= 1 && n <= 1 << 24 && k >= 0 && k <= n && T >= 1 && (indices ? stride >= k : T == 1),
                 "micv_fundamental_ls_dev: need 0 <= k <= n, T >= 1, stride >= k (n %d, k %d, T %d, stride %d)", n, k,
                 T, stride);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    MICV_HIP(hipMemsetAsync(status, 0, 4, s));
    if (flags & MICV_GEOM_F64)
        fund_ls_kernel<double, float><<<grid_for(ctx, T), 64 * kWaves, 0, s>>>(ptsA, ptsB, n, indices, stride, k, T, F,
                                                                              nullptr, status);
    else
        fund_ls_kernel<float, float><<<grid_for(ctx, T), 64 * kWaves, 0, s>>>(ptsA, ptsB, n, indices, stride, k, T, F,
                                                                             nullptr, status);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_fundamental_rank_reduce_dev(micv_ctx *ctx, const float *F, int T, uint32_t flags, float *out,
                                     micv_stream stream) {
    MICV_REQUIRE(ctx && F && out, "micv_fundamental_rank_reduce_dev: null argument");
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64) && T >= 1, "micv_fundamental_rank_reduce_dev: unknown flags %u or T = %d < 1",
                 flags, T);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & MICV_GEOM_F64) return rank_launch<double>(ctx, s, F, T, out);
    return rank_launch<float>(ctx, s, F, T, out);
}

int micv_fundamental_normalized_dev(micv_ctx *ctx, const float *ptsA, const float *ptsB, int n, uint32_t flags,
                                    float *Ta, float *Tb, float *Fhat, float *F, micv_stream stream) {
    MICV_REQUIRE(ctx && ptsA && ptsB && Ta && Tb && Fhat && F, "micv_fundamental_normalized_dev: null argument");
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64) && n >= 1 && n <= 1 << 24,
                 "micv_fundamental_normalized_dev: unknown flags %u or n = %d outside 1 .. 2^24", flags, n);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & MICV_GEOM_F64) return normalized_launch<double>(ctx, s, ptsA, ptsB, n, Ta, Tb, Fhat, F);
    return normalized_launch<float>(ctx, s, ptsA, ptsB, n, Ta, Tb, Fhat, F);
}

int micv_epipolar_endpoints_dev(micv_ctx *ctx, const float *F, const float *pts, int n, int side, int rows, int cols,
                                uint32_t flags, float *out, micv_stream stream) {
    MICV_REQUIRE(ctx && F && pts && out, "micv_epipolar_endpoints_dev: null argument");
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64) && n >= 1 && n <= 1 << 28 && (side == 0 || side == 1) && rows >= 1 &&
                     cols >= 1,
                 "micv_epipolar_endpoints_dev: bad flags %u, n %d, side %d or image size %d x %d", flags, n, side, rows,
                 cols);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & MICV_GEOM_F64)
        epipolar_kernel<double><<<cdiv((unsigned)n, 256), 256, 0, s>>>(F, pts, n, side, rows, cols, out);
    else
        epipolar_kernel<float><<<cdiv((unsigned)n, 256), 256, 0, s>>>(F, pts, n, side, rows, cols, out);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_camera_center_dev(micv_ctx *ctx, const float *M, int T, uint32_t flags, float *center, micv_stream stream) {
    MICV_REQUIRE(ctx && M && center, "micv_camera_center_dev: null argument");
    MICV_REQUIRE(!(flags & ~MICV_GEOM_F64) && T >= 1, "micv_camera_center_dev: unknown flags %u or T = %d < 1", flags, T);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (flags & MICV_GEOM_F64)
        camera_center_kernel<double><<<cdiv((unsigned)T, 256), 256, 0, s>>>(M, T, center);
    else
        camera_center_kernel<float><<<cdiv((unsigned)T, 256), 256, 0, s>>>(M, T, center);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

}  // extern "C"
