// pf.hip -- ParticleFilter (ps6_cpp/lib/ParticleFilter.cpp) on the device, and its host-side generator.
//
// Everything stochastic in the reference is fixed at construction (each of displaceParticles,
// resampleMultinomial and genParticles builds a fresh cv::RNG), so create() draws the displacement
// table (n gaussian pairs), the resampling table (n uniforms) and the initial particles once on the
// host and uploads them.  A tick is then three launches on one stream, no host sync, no branch:
//   pf_score_kernel     one workgroup per particle: displace, bounds test, patch score (exact integer
//                       sums; MSE in 64-bit lane sums, histograms in per-wave LDS bins), double sim.
//   pf_resample_kernel  one workgroup: the sequential double simSum and float prefix sum on lane 0 out of
//                       LDS, weights and one binary search per particle in parallel, the sequential
//                       float mean / variance on lane 0, the state out.
//   pf_model_kernel     one workgroup: the blend at the rounded mean; in histogram mode the blend's
//                       normalized histogram becomes the model histogram.
// Arithmetic: mi_cv.h "ps6: particle filter" and DESIGN.md section 2.  -ffp-contract=off: no fma here.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <unordered_set>
#include <vector>

#include "common.hpp"
#include "cv_rng.hpp"
#include "pf.hpp"

namespace micv {
namespace {

constexpr int kBins = 32;
constexpr int kScoreThreads = 256;  // 4 waves: wave w scores patch rows w, w + 4, ...
constexpr int kTailThreads = 1024;
constexpr int kMaxN = MICV_PF_MAX_PARTICLES;

// ---------------------------------------------------------------- arithmetic shared by host and device

// pow2i, pf_exp (the library's double exp): cv_rng.hpp.

// cvRound of a float: nearest, halves to even (the caller keeps |v| < 2^24 + 1).
__device__ inline int cv_round(float v) { return (int)rintf(v); }

// ------------------------------------------------------------------------------------------ device

struct PatchGeom {
    const uint8_t *frame;
    size_t stride;
    int rows, cols, ch;    // frame
    int mrows, mcols;      // patch
    int x0, y0;            // frame coordinates of the patch's top-left pixel (may lie outside)
};

// Byte b of patch row r (b < mcols * ch), BORDER_REPLICATE outside the frame.
__device__ inline unsigned patch_byte(const PatchGeom &g, const uint8_t *row, int b, bool inside) {
    if (inside) return row[(size_t)g.x0 * g.ch + b];
    const int j = g.ch == 1 ? b : b / 3;
    const int c = b - j * g.ch;
    return row[(size_t)clampi(g.x0 + j, 0, g.cols - 1) * g.ch + c];
}

// One wave's sum of v into red[wave].
__device__ inline void wave_sum_u64(unsigned long long v, unsigned long long *red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
}

// Normalize one channel's counts (cv::normalize NORM_L2 as mi_cv.h states) into out[32].
__device__ inline void l2_normalize(const unsigned *h, float *out) {
    unsigned long long ss = 0;
    for (int b = 0; b < kBins; b++) ss += (unsigned long long)h[b] * h[b];  // exact (< 2^53)
    const double inv = 1.0 / sqrt((double)ss);
    for (int b = 0; b < kBins; b++) out[b] = (float)((double)h[b] * inv);
}

// Displace particle blockIdx.x, test it, score its patch: moved[i], sim[i] (0 outside the frame).
__global__ void __launch_bounds__(kScoreThreads)
pf_score_kernel(const uint8_t *__restrict__ frame, size_t stride, int rows, int cols, int ch, int mrows, int mcols,
                int mode, uint32_t flags, double mse_sigma, const float2 *__restrict__ parts,
                const double2 *__restrict__ disp, const uint8_t *__restrict__ model, const float *__restrict__ mhist,
                float2 *__restrict__ moved, double *__restrict__ sim) {
    __shared__ unsigned bins[kScoreThreads / 64][3 * kBins];
    __shared__ unsigned long long red[kScoreThreads / 64];
    const int i = blockIdx.x;
    const float2 p0 = parts[i];
    const double2 g = disp[i];
    const float px = (float)((double)p0.x + g.x), py = (float)((double)p0.y + g.y);
    if (threadIdx.x == 0) moved[i] = make_float2(px, py);
    if (!(px >= 0.f && px < (float)cols && py >= 0.f && py < (float)rows)) {  // (finite tables: never NaN)
        if (threadIdx.x == 0) sim[i] = 0.0;
        return;
    }
    PatchGeom pg{frame, stride, rows, cols, ch, mrows, mcols, cv_round(px) - (mcols + 1) / 2,
                 cv_round(py) - (mrows + 1) / 2};
    const bool inside = pg.x0 >= 0 && pg.x0 + mcols <= cols;
    const int rb = mcols * ch, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (mode == MICV_PF_MSE) {
        const bool sgn = flags & MICV_PF_MSE_SIGNED;
        unsigned long long acc = 0;
        for (int r = wave; r < mrows; r += kScoreThreads / 64) {
            const uint8_t *row = frame + (size_t)clampi(pg.y0 + r, 0, rows - 1) * stride;
            const uint8_t *mrow = model + (size_t)r * rb;
            for (int b = lane; b < rb; b += 64) {
                const int m = mrow[b], c = (int)patch_byte(pg, row, b, inside);
                const int d = m - c;
                acc += (unsigned)(sgn ? d * d : (d > 0 ? min(d * d, 255) : 0));
            }
        }
        wave_sum_u64(acc, red);
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long s = 0;
            for (int w = 0; w < kScoreThreads / 64; w++) s += red[w];
            const double mse = (double)s / (double)(mrows * mcols);
            sim[i] = pf_exp(-mse / (2 * mse_sigma * mse_sigma));
        }
        return;
    }
    // MICV_PF_HIST
    for (int k = threadIdx.x; k < (kScoreThreads / 64) * 3 * kBins; k += kScoreThreads) (&bins[0][0])[k] = 0;
    __syncthreads();
    for (int r = wave; r < mrows; r += kScoreThreads / 64) {
        const uint8_t *row = frame + (size_t)clampi(pg.y0 + r, 0, rows - 1) * stride;
        for (int b = lane; b < rb; b += 64) {
            const int c = ch == 1 ? 0 : b % 3;
            atomicAdd(&bins[wave][c * kBins + (patch_byte(pg, row, b, inside) >> 3)], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < ch * kBins) {
        unsigned s = 0;
        for (int w = 0; w < kScoreThreads / 64; w++) s += bins[w][threadIdx.x];
        bins[0][threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double comp = 0;
        for (int c = 0; c < ch; c++) {
            float h[kBins];
            l2_normalize(&bins[0][c * kBins], h);
            double chi = 0;
            for (int b = 0; b < kBins; b++) {
                const float a = mhist[c * kBins + b];
                const float d = a - h[b];
                if (fabs((double)a) > DBL_EPSILON) chi += (double)d * (double)d / (double)a;
            }
            comp += chi;
        }
        comp /= (double)ch;
        sim[i] = pf_exp(-comp);
    }
}

// Weights, resampling and the estimate: one workgroup of kTailThreads.
__global__ void __launch_bounds__(kTailThreads)
pf_resample_kernel(int n, const double *__restrict__ sim, const float *__restrict__ uni,
                   const float2 *__restrict__ moved, float *__restrict__ weights, float2 *__restrict__ parts,
                   micv_pf_state *__restrict__ state, micv_pf_state *__restrict__ state_out) {
    __shared__ double s_sim[kMaxN];
    __shared__ float s_cum[kMaxN];
    // the resampled particles, written only after the last read of s_sim (48 KiB in all): lane 0's sequential
    // estimate reads LDS, not one dependent global load per particle
    float2 *s_part = reinterpret_cast<float2 *>(s_sim);
    __shared__ double s_sum;
    __shared__ unsigned s_status;
    for (int i = threadIdx.x; i < n; i += kTailThreads) s_sim[i] = sim[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0;  // updateParticles' simSum: the double similarities in particle order
        for (int i = 0; i < n; i++) sum += s_sim[i];
        s_sum = sum;
        s_status = (sum == 0.0 || !isfinite(sum)) ? MICV_PF_STATUS_NO_WEIGHT : 0u;
    }
    __syncthreads();
    const double sum = s_sum;
    const bool keep = s_status & MICV_PF_STATUS_NO_WEIGHT;
    for (int i = threadIdx.x; i < n; i += kTailThreads) {
        const float w0 = (float)s_sim[i];
        const float w = keep ? w0 : (float)((double)w0 / sum);
        weights[i] = w;
        s_cum[i] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0 && !keep) {  // resampleMultinomial's cumulative sum, sequential float
        float c = s_cum[0];
        for (int i = 1; i < n; i++) {
            c = s_cum[i] + c;
            s_cum[i] = c;
        }
    }
    __syncthreads();
    bool clamped = false;
    for (int i = threadIdx.x; i < n; i += kTailThreads) {
        int idx = i;
        if (!keep) {
            const float u = uni[i];
            int lo = 0, hi = n;  // std::upper_bound: the first cum > u
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (u < s_cum[mid]) hi = mid;
                else lo = mid + 1;
            }
            clamped |= lo == n;
            idx = lo < n ? lo : n - 1;
        }
        const float2 p = moved[idx];
        s_part[i] = p;
        parts[i] = p;
    }
    if (__any(clamped) && (threadIdx.x & 63) == 0) atomicOr(&s_status, MICV_PF_STATUS_CLAMPED);
    __syncthreads();
    if (threadIdx.x == 0) {  // estimateState, sequential float sums in particle order
        float xm = 0.f, ym = 0.f, xv = 0.f, yv = 0.f;
        for (int i = 0; i < n; i++) {
            const float2 p = s_part[i];
            xm += p.x;
            ym += p.y;
        }
        xm /= (float)n;
        ym /= (float)n;
        for (int i = 0; i < n; i++) {
            const float2 p = s_part[i];
            xv += (p.x - xm) * (p.x - xm);
            yv += (p.y - ym) * (p.y - ym);
        }
        xv /= (float)n;
        yv /= (float)n;
        const micv_pf_state st{xm, ym, xv, yv, s_status};
        *state = st;
        if (state_out) *state_out = st;
    }
}

// updateModel at the rounded estimate: one workgroup of kTailThreads.
__global__ void __launch_bounds__(kTailThreads)
pf_model_kernel(const uint8_t *__restrict__ frame, size_t stride, int rows, int cols, int ch, int mrows, int mcols,
                int mode, float fa, float fb, const micv_pf_state *__restrict__ state,
                const uint8_t *__restrict__ model0, uint8_t *__restrict__ model, float *__restrict__ mhist) {
    __shared__ unsigned bins[kTailThreads / 64][3 * kBins];
    const float lim = 16777216.f;
    const float ex = fminf(fmaxf(state->x, -lim), lim), ey = fminf(fmaxf(state->y, -lim), lim);
    PatchGeom pg{frame, stride, rows, cols, ch, mrows, mcols, cv_round(ex) - (mcols + 1) / 2,
                 cv_round(ey) - (mrows + 1) / 2};
    const bool inside = pg.x0 >= 0 && pg.x0 + mcols <= cols;
    const bool hist = mode == MICV_PF_HIST;
    const uint8_t *old = hist ? model0 : model;
    const int rb = mcols * ch, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (hist) {
        for (int k = threadIdx.x; k < (kTailThreads / 64) * 3 * kBins; k += kTailThreads) (&bins[0][0])[k] = 0;
        __syncthreads();
    }
    for (int r = wave; r < mrows; r += kTailThreads / 64) {
        const uint8_t *row = frame + (size_t)clampi(pg.y0 + r, 0, rows - 1) * stride;
        for (int b = lane; b < rb; b += 64) {
            const size_t k = (size_t)r * rb + b;
            const float t = (float)patch_byte(pg, row, b, inside) * fa + (float)old[k] * fb;
            const int v = clampi((int)rintf(t), 0, 255);  // saturate_cast<uchar>(float): cvRound, then clamp
            model[k] = (uint8_t)v;
            if (hist) atomicAdd(&bins[wave][(ch == 1 ? 0 : b % 3) * kBins + (v >> 3)], 1u);
        }
    }
    if (!hist) return;
    __syncthreads();
    if (threadIdx.x < ch * kBins) {
        unsigned s = 0;
        for (int w = 0; w < kTailThreads / 64; w++) s += bins[w][threadIdx.x];
        bins[0][threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < ch) l2_normalize(&bins[0][threadIdx.x * kBins], mhist + threadIdx.x * kBins);
}

// -------------------------------------------------------------------------------------------- host

// CvRng, Ziggurat (cv::RNG as mi_cv.h restates it): cv_rng.hpp.

struct PairHash {
    size_t operator()(const std::pair<float, float> &p) const {
        // bit patterns with -0 folded onto +0, so that float == decides (NaN never occurs here)
        const uint32_t a = p.first == 0.f ? 0u : __builtin_bit_cast(uint32_t, p.first);
        const uint32_t b = p.second == 0.f ? 0u : __builtin_bit_cast(uint32_t, p.second);
        return std::hash<uint64_t>()((uint64_t)a << 32 | b);
    }
};

// genParticles (ParticleFilter.cpp:248-283), exact duplicates drawn again; false when n distinct pairs
// do not come within 64 n + 4096 draws.
bool gen_particles(uint64_t seed, int n, bool uniform, float xmax, float ymax, double sigma, float cx, float cy,
                   std::vector<float2> &out) {
    CvRng rng(seed);
    std::unordered_set<std::pair<float, float>, PairHash> seen;
    out.clear();
    const long long max_tries = 64LL * n + 4096;
    for (long long t = 0; t < max_tries && (int)out.size() < n; t++) {
        float x, y;
        if (uniform) {
            x = rng.uniform(0.f, xmax);
            y = rng.uniform(0.f, ymax);
        } else {
            x = (float)(rng.gaussian(sigma) + (double)cx);
            y = (float)(rng.gaussian(sigma) + (double)cy);
        }
        if (seen.emplace(x, y).second) out.push_back(make_float2(x, y));
    }
    return (int)out.size() == n;
}

// Counts of one channel (host) -> normalized histogram, exactly as the device's l2_normalize.
void host_hist(const uint8_t *patch, int mrows, int mcols, int ch, float *out) {
    for (int c = 0; c < ch; c++) {
        unsigned h[kBins] = {0};
        for (size_t k = c; k < (size_t)mrows * mcols * ch; k += ch) h[patch[k] >> 3]++;
        unsigned long long ss = 0;
        for (int b = 0; b < kBins; b++) ss += (unsigned long long)h[b] * h[b];
        const double inv = 1.0 / std::sqrt((double)ss);
        for (int b = 0; b < kBins; b++) out[c * kBins + b] = (float)((double)h[b] * inv);
    }
}

int enqueue_tick(micv_pf *pf, const uint8_t *frame, size_t stride, hipStream_t s, micv_pf_state *state_out) {
    pf_score_kernel<<<pf->n, kScoreThreads, 0, s>>>(frame, stride, pf->rows, pf->cols, pf->ch, pf->mrows, pf->mcols,
                                                    pf->mode, pf->flags, pf->mse_sigma, pf->parts, pf->disp,
                                                    pf->model, pf->hist, pf->moved, pf->sim);
    MICV_LAUNCH_CHECK();
    pf_resample_kernel<<<1, kTailThreads, 0, s>>>(pf->n, pf->sim, pf->uni, pf->moved, pf->weights, pf->parts,
                                                  pf->state, state_out);
    MICV_LAUNCH_CHECK();
    pf_model_kernel<<<1, kTailThreads, 0, s>>>(frame, stride, pf->rows, pf->cols, pf->ch, pf->mrows, pf->mcols,
                                               pf->mode, pf->fa, pf->fb, pf->state, pf->model0, pf->model, pf->hist);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int frame_buffers(micv_pf *pf) {
    for (auto &b : pf->frame_buf)
        if (!b) MICV_HIP(hipMalloc(&b, pf->frame_bytes()));
    return MICV_OK;
}

}  // namespace

// For ps6.hip (pf.hpp).
int pf_enqueue_tick(micv_pf *pf, const uint8_t *frame, size_t stride, hipStream_t s, micv_pf_state *state_out) {
    return enqueue_tick(pf, frame, stride, s, state_out);
}
int pf_frame_buffers(micv_pf *pf) { return frame_buffers(pf); }

}  // namespace micv

using namespace micv;

extern "C" {

int micv_pf_create(micv_ctx *ctx, const uint8_t *model, int mrows, int mcols, size_t mstride, int channels,
                   int img_rows, int img_cols, int n, int mode, double mse_sigma, double sample_sigma,
                   float init_x, float init_y, double alpha, uint32_t flags, uint64_t seed, micv_pf **out) {
    MICV_REQUIRE(ctx && model && out, "micv_pf_create: null argument");
    *out = nullptr;
    MICV_REQUIRE(channels == 1 || channels == 3, "micv_pf_create: %d channels, need 1 or 3", channels);
    MICV_REQUIRE(img_rows >= 1 && img_cols >= 1 && (size_t)img_rows * img_cols * channels <= ((size_t)1 << 31),
                 "micv_pf_create: frame %d x %d", img_rows, img_cols);
    MICV_REQUIRE(mrows >= 1 && mcols >= 1 && mrows <= img_rows && mcols <= img_cols,
                 "micv_pf_create: model %d x %d does not fit in the %d x %d frame", mrows, mcols, img_rows, img_cols);
    MICV_REQUIRE(mstride >= (size_t)mcols * channels, "micv_pf_create: model stride %zu", mstride);
    MICV_REQUIRE(n >= 1 && n <= MICV_PF_MAX_PARTICLES, "micv_pf_create: n = %d outside 1 .. %d", n,
                 MICV_PF_MAX_PARTICLES);
    MICV_REQUIRE(mode == MICV_PF_MSE || mode == MICV_PF_HIST, "micv_pf_create: mode %d", mode);
    MICV_REQUIRE(mode != MICV_PF_MSE || (mse_sigma > 0 && std::isfinite(mse_sigma)),
                 "micv_pf_create: mse_sigma %g, need 0 < sigma < inf", mse_sigma);
    MICV_REQUIRE(std::isfinite(sample_sigma) && sample_sigma >= 0 && std::isfinite(alpha) &&
                     std::isfinite(init_x) && std::isfinite(init_y),
                 "micv_pf_create: sample_sigma %g, alpha %g or the initial position is not finite", sample_sigma,
                 alpha);
    MICV_REQUIRE((flags & ~MICV_PF_MSE_SIGNED) == 0, "micv_pf_create: unknown flags 0x%x", flags);

    const bool uniform = init_x == -1.f && init_y == -1.f;
    std::vector<float2> init;
    if (!gen_particles(seed, n, uniform, (float)img_cols, (float)img_rows, sample_sigma,
                       init_x + (float)mcols / 2.f, init_y + (float)mrows / 2.f, init))
        MICV_REQUIRE(false, "micv_pf_create: cannot draw %d distinct initial particles (sample_sigma %g)", n,
                     sample_sigma);
    std::vector<double2> disp(n);
    {
        CvRng rng(seed);
        for (int i = 0; i < n; i++) {
            disp[i].x = rng.gaussian(sample_sigma);
            disp[i].y = rng.gaussian(sample_sigma);
        }
    }
    std::vector<float> uni(n);
    {
        CvRng rng(seed);
        for (int i = 0; i < n; i++) uni[i] = rng.uniform(0.f, 1.f);
    }
    std::vector<uint8_t> patch((size_t)mrows * mcols * channels);
    for (int r = 0; r < mrows; r++)
        std::memcpy(&patch[(size_t)r * mcols * channels], model + (size_t)r * mstride, (size_t)mcols * channels);
    std::vector<float> hist(3 * kBins, 0.f);
    if (mode == MICV_PF_HIST) host_hist(patch.data(), mrows, mcols, channels, hist.data());
    std::vector<float> w(n, 1.f / (float)n);

    MICV_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<micv_pf> pf(new micv_pf);
    pf->device = ctx->device;
    pf->mrows = mrows, pf->mcols = mcols, pf->ch = channels, pf->rows = img_rows, pf->cols = img_cols, pf->n = n;
    pf->mode = mode, pf->flags = flags, pf->mse_sigma = mse_sigma;
    pf->fa = (float)alpha, pf->fb = (float)(1.0 - alpha);
    MICV_HIP(hipMalloc(&pf->parts, n * sizeof(float2)));
    MICV_HIP(hipMalloc(&pf->moved, n * sizeof(float2)));
    MICV_HIP(hipMalloc(&pf->disp, n * sizeof(double2)));
    MICV_HIP(hipMalloc(&pf->uni, n * sizeof(float)));
    MICV_HIP(hipMalloc(&pf->sim, n * sizeof(double)));
    MICV_HIP(hipMalloc(&pf->weights, n * sizeof(float)));
    MICV_HIP(hipMalloc(&pf->model, patch.size()));
    MICV_HIP(hipMalloc(&pf->model0, patch.size()));
    MICV_HIP(hipMalloc(&pf->hist, hist.size() * sizeof(float)));
    MICV_HIP(hipMalloc(&pf->state, sizeof(micv_pf_state)));
    MICV_HIP(hipMemcpy(pf->parts, init.data(), n * sizeof(float2), hipMemcpyHostToDevice));
    MICV_HIP(hipMemcpy(pf->moved, init.data(), n * sizeof(float2), hipMemcpyHostToDevice));
    MICV_HIP(hipMemcpy(pf->disp, disp.data(), n * sizeof(double2), hipMemcpyHostToDevice));
    MICV_HIP(hipMemcpy(pf->uni, uni.data(), n * sizeof(float), hipMemcpyHostToDevice));
    MICV_HIP(hipMemcpy(pf->weights, w.data(), n * sizeof(float), hipMemcpyHostToDevice));
    MICV_HIP(hipMemcpy(pf->model, patch.data(), patch.size(), hipMemcpyHostToDevice));
    MICV_HIP(hipMemcpy(pf->model0, patch.data(), patch.size(), hipMemcpyHostToDevice));
    MICV_HIP(hipMemcpy(pf->hist, hist.data(), hist.size() * sizeof(float), hipMemcpyHostToDevice));
    MICV_HIP(hipMemset(pf->sim, 0, n * sizeof(double)));
    MICV_HIP(hipMemset(pf->state, 0, sizeof(micv_pf_state)));
    *out = pf.release();
    return MICV_OK;
}

void micv_pf_destroy(micv_pf *pf) {
    if (!pf) return;
    (void)hipSetDevice(pf->device);
    (void)hipDeviceSynchronize();  // nothing enqueued on its buffers may still run
    delete pf;
}

int micv_pf_tick_dev(micv_pf *pf, const uint8_t *frame, size_t stride, micv_stream stream,
                     micv_pf_state *state_dev) {
    MICV_REQUIRE(pf && frame, "micv_pf_tick_dev: null argument");
    MICV_REQUIRE(stride >= (size_t)pf->cols * pf->ch, "micv_pf_tick_dev: stride %zu < %d", stride, pf->cols * pf->ch);
    MICV_HIP(hipSetDevice(pf->device));
    return enqueue_tick(pf, frame, stride, static_cast<hipStream_t>(stream), state_dev);
}

int micv_pf_tick_host(micv_pf *pf, const uint8_t *frame, size_t stride, micv_pf_state *state) {
    MICV_REQUIRE(pf && frame && state, "micv_pf_tick_host: null argument");
    MICV_REQUIRE(stride >= (size_t)pf->cols * pf->ch, "micv_pf_tick_host: stride %zu < %d", stride,
                 pf->cols * pf->ch);
    MICV_HIP(hipSetDevice(pf->device));
    MICV_TRY(frame_buffers(pf));
    const size_t rb = (size_t)pf->cols * pf->ch;
    hipStream_t s = nullptr;
    MICV_HIP(hipMemcpy2DAsync(pf->frame_buf[0], rb, frame, stride, rb, pf->rows, hipMemcpyHostToDevice, s));
    MICV_TRY(enqueue_tick(pf, pf->frame_buf[0], rb, s, nullptr));
    MICV_HIP(hipMemcpyAsync(state, pf->state, sizeof(micv_pf_state), hipMemcpyDeviceToHost, s));
    MICV_HIP(hipStreamSynchronize(s));
    return MICV_OK;
}

int micv_pf_particles_dev(micv_pf *pf, float *xy, micv_stream stream) {
    MICV_REQUIRE(pf && xy, "micv_pf_particles_dev: null argument");
    MICV_HIP(hipSetDevice(pf->device));
    MICV_HIP(hipMemcpyAsync(xy, pf->parts, pf->n * sizeof(float2), hipMemcpyDeviceToDevice,
                            static_cast<hipStream_t>(stream)));
    return MICV_OK;
}

int micv_pf_particles_host(micv_pf *pf, float *xy) {
    MICV_REQUIRE(pf && xy, "micv_pf_particles_host: null argument");
    MICV_HIP(hipSetDevice(pf->device));
    MICV_HIP(hipMemcpy(xy, pf->parts, pf->n * sizeof(float2), hipMemcpyDeviceToHost));
    return MICV_OK;
}

int micv_pf_weights_dev(micv_pf *pf, float *w, micv_stream stream) {
    MICV_REQUIRE(pf && w, "micv_pf_weights_dev: null argument");
    MICV_HIP(hipSetDevice(pf->device));
    MICV_HIP(hipMemcpyAsync(w, pf->weights, pf->n * sizeof(float), hipMemcpyDeviceToDevice,
                            static_cast<hipStream_t>(stream)));
    return MICV_OK;
}

int micv_pf_weights_host(micv_pf *pf, float *w) {
    MICV_REQUIRE(pf && w, "micv_pf_weights_host: null argument");
    MICV_HIP(hipSetDevice(pf->device));
    MICV_HIP(hipMemcpy(w, pf->weights, pf->n * sizeof(float), hipMemcpyDeviceToHost));
    return MICV_OK;
}

int micv_pf_model_host(micv_pf *pf, uint8_t *patch, float *hist) {
    MICV_REQUIRE(pf, "micv_pf_model_host: null argument");
    MICV_HIP(hipSetDevice(pf->device));
    if (patch) MICV_HIP(hipMemcpy(patch, pf->model, pf->patch_bytes(), hipMemcpyDeviceToHost));
    if (hist) MICV_HIP(hipMemcpy(hist, pf->hist, (size_t)pf->ch * kBins * sizeof(float), hipMemcpyDeviceToHost));
    return MICV_OK;
}

int micv_pf_track_seq_host(micv_pf *pf, const uint8_t *const *frames, int nframes, size_t stride,
                           micv_pf_state *states, float *particles) {
    MICV_REQUIRE(pf && frames && states && nframes >= 1, "micv_pf_track_seq_host: bad argument");
    MICV_REQUIRE(stride >= (size_t)pf->cols * pf->ch, "micv_pf_track_seq_host: stride %zu < %d", stride,
                 pf->cols * pf->ch);
    for (int t = 0; t < nframes; t++) MICV_REQUIRE(frames[t], "micv_pf_track_seq_host: frame %d is null", t);
    MICV_HIP(hipSetDevice(pf->device));
    MICV_TRY(frame_buffers(pf));
    const size_t rb = (size_t)pf->cols * pf->ch, pbytes = (size_t)pf->n * sizeof(float2);
    struct Scope {  // released on every way out, after everything enqueued has finished
        hipStream_t up = nullptr, run = nullptr;
        std::vector<hipEvent_t> ev;
        void *st = nullptr, *pt = nullptr;
        ~Scope() {
            for (hipStream_t s : {up, run})
                if (s) (void)hipStreamSynchronize(s);
            for (hipEvent_t e : ev) (void)hipEventDestroy(e);
            for (hipStream_t s : {up, run})
                if (s) (void)hipStreamDestroy(s);
            if (st) (void)hipFree(st);
            if (pt) (void)hipFree(pt);
        }
    } sc;
    MICV_HIP(hipStreamCreateWithFlags(&sc.up, hipStreamNonBlocking));
    MICV_HIP(hipStreamCreateWithFlags(&sc.run, hipStreamNonBlocking));
    MICV_HIP(hipMalloc(&sc.st, (size_t)nframes * sizeof(micv_pf_state)));
    if (particles) MICV_HIP(hipMalloc(&sc.pt, (size_t)nframes * pbytes));
    std::vector<hipEvent_t> ev_up(nframes), ev_tick(nframes);
    sc.ev.reserve(2 * (size_t)nframes);
    for (auto *v : {&ev_up, &ev_tick})
        for (auto &e : *v) {
            MICV_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            sc.ev.push_back(e);
        }
    micv_pf_state *dst = static_cast<micv_pf_state *>(sc.st);
    auto upload = [&](int t) -> int {
        if (t >= 2) MICV_HIP(hipStreamWaitEvent(sc.up, ev_tick[t - 2], 0));  // its buffer's last reader
        MICV_HIP(hipMemcpy2DAsync(pf->frame_buf[t & 1], rb, frames[t], stride, rb, pf->rows, hipMemcpyHostToDevice,
                                  sc.up));
        MICV_HIP(hipEventRecord(ev_up[t], sc.up));
        return MICV_OK;
    };
    MICV_TRY(upload(0));
    for (int t = 0; t < nframes; t++) {
        MICV_HIP(hipStreamWaitEvent(sc.run, ev_up[t], 0));
        MICV_TRY(enqueue_tick(pf, pf->frame_buf[t & 1], rb, sc.run, dst + t));
        if (particles)
            MICV_HIP(hipMemcpyAsync(static_cast<char *>(sc.pt) + (size_t)t * pbytes, pf->parts, pbytes,
                                    hipMemcpyDeviceToDevice, sc.run));
        MICV_HIP(hipEventRecord(ev_tick[t], sc.run));
        if (t + 1 < nframes) MICV_TRY(upload(t + 1));  // (a pageable copy holds this thread: tick t runs meanwhile)
    }
    MICV_HIP(hipMemcpyAsync(states, sc.st, (size_t)nframes * sizeof(micv_pf_state), hipMemcpyDeviceToHost, sc.run));
    if (particles)
        MICV_HIP(hipMemcpyAsync(particles, sc.pt, (size_t)nframes * pbytes, hipMemcpyDeviceToHost, sc.run));
    MICV_HIP(hipStreamSynchronize(sc.run));
    return MICV_OK;
}

}  // extern "C"
