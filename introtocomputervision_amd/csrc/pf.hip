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
// A group (micv_pf_group) ticks up to 64 filters in the same three launches: each stage is written once, and the single
// tick's kernels and the group's are two entries into it, so a member's bytes cannot depend on the entry.  A group owns
// a device table of member descriptors and nothing else; the frames travel in the launch arguments.
// Arithmetic: mi_cv.h "ps6: particle filter" and DESIGN.md section 2.  -ffp-contract=off: no fma here.
#include <algorithm>
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

// The stages of a tick, each written once; the single tick's kernels and the group's (below) are two entries into each.
// Resampling is a function.  Scoring and the model update are text (pf_score_body.hpp, pf_model_body.hpp): as inline
// functions they changed the single tick's register allocation (profiles/pf_group/resources.txt), as text they do not.

// Weights, resampling and the estimate: one workgroup of kTailThreads.
__device__ __forceinline__ void
pf_resample_body(int n, const double *__restrict__ sim, const float *__restrict__ uni,
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

// The single tick: particle blockIdx.x / one workgroup / one workgroup.
__global__ void __launch_bounds__(kScoreThreads)
pf_score_kernel(const uint8_t *__restrict__ frame, size_t stride, int rows, int cols, int ch, int mrows, int mcols,
                int mode, uint32_t flags, double mse_sigma, const float2 *__restrict__ parts,
                const double2 *__restrict__ disp, const uint8_t *__restrict__ model, const float *__restrict__ mhist,
                float2 *__restrict__ moved, double *__restrict__ sim) {
    const int i = blockIdx.x;
#include "pf_score_body.hpp"
}

__global__ void __launch_bounds__(kTailThreads)
pf_resample_kernel(int n, const double *__restrict__ sim, const float *__restrict__ uni,
                   const float2 *__restrict__ moved, float *__restrict__ weights, float2 *__restrict__ parts,
                   micv_pf_state *__restrict__ state, micv_pf_state *__restrict__ state_out) {
    pf_resample_body(n, sim, uni, moved, weights, parts, state, state_out);
}

__global__ void __launch_bounds__(kTailThreads)
pf_model_kernel(const uint8_t *__restrict__ frame, size_t stride, int rows, int cols, int ch, int mrows, int mcols,
                int mode, float fa, float fb, const micv_pf_state *__restrict__ state,
                const uint8_t *__restrict__ model0, uint8_t *__restrict__ model, float *__restrict__ mhist) {
#include "pf_model_body.hpp"
}

// The group's tick: member blockIdx.y of the descriptor table `members`, its frame out of the launch arguments (64 x 16
// bytes at the cap).  Everything a workgroup takes from the table and from `f` is uniform over the workgroup.
struct GroupFrames {
    const uint8_t *frame[MICV_PF_GROUP_MAX];
    size_t stride[MICV_PF_GROUP_MAX];
};

// Grid (max n, count): a workgroup past its member's n returns having read the descriptor alone.
__global__ void __launch_bounds__(kScoreThreads)
pf_group_score_kernel(const PfMember *__restrict__ members, const GroupFrames f) {
    const PfMember &m = members[blockIdx.y];
    const int i = blockIdx.x;
    if (i >= m.n) return;
    const uint8_t *__restrict__ frame = f.frame[blockIdx.y];
    const size_t stride = f.stride[blockIdx.y];
    const int rows = m.rows, cols = m.cols, ch = m.ch, mrows = m.mrows, mcols = m.mcols, mode = m.mode;
    const uint32_t flags = m.flags;
    const double mse_sigma = m.mse_sigma;
    const float2 *__restrict__ parts = m.parts;
    const double2 *__restrict__ disp = m.disp;
    const uint8_t *__restrict__ model = m.model;
    const float *__restrict__ mhist = m.hist;
    float2 *__restrict__ moved = m.moved;
    double *__restrict__ sim = m.sim;
#include "pf_score_body.hpp"
}

// Grid (count): one workgroup per member.  states_out: count entries or NULL.
__global__ void __launch_bounds__(kTailThreads)
pf_group_resample_kernel(const PfMember *__restrict__ members, micv_pf_state *__restrict__ states_out) {
    const int k = blockIdx.x;
    const PfMember &m = members[k];
    pf_resample_body(m.n, m.sim, m.uni, m.moved, m.weights, m.parts, m.state, states_out ? states_out + k : nullptr);
}

__global__ void __launch_bounds__(kTailThreads)
pf_group_model_kernel(const PfMember *__restrict__ members, const GroupFrames f) {
    const PfMember &m = members[blockIdx.x];
    const uint8_t *__restrict__ frame = f.frame[blockIdx.x];
    const size_t stride = f.stride[blockIdx.x];
    const int rows = m.rows, cols = m.cols, ch = m.ch, mrows = m.mrows, mcols = m.mcols, mode = m.mode;
    const float fa = m.fa, fb = m.fb;
    const micv_pf_state *__restrict__ state = m.state;
    const uint8_t *__restrict__ model0 = m.model0;
    uint8_t *__restrict__ model = m.model;
    float *__restrict__ mhist = m.hist;
#include "pf_model_body.hpp"
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

// A member's row as of NOW: the buffer pointers and the scalars are copied, and a group uploads its rows once, at create.
// That holds because no micv_pf call reallocates a buffer or changes n, mode, flags, sigma or alpha after micv_pf_create;
// a setter or a reallocation added to micv_pf later must refresh (or invalidate) the tables of the groups that hold it.
PfMember describe(const micv_pf *pf) {
    PfMember m{};
    m.rows = pf->rows, m.cols = pf->cols, m.ch = pf->ch, m.mrows = pf->mrows, m.mcols = pf->mcols, m.n = pf->n;
    m.mode = pf->mode, m.flags = pf->flags, m.mse_sigma = pf->mse_sigma, m.fa = pf->fa, m.fb = pf->fb;
    m.parts = pf->parts, m.moved = pf->moved, m.disp = pf->disp, m.uni = pf->uni, m.sim = pf->sim;
    m.weights = pf->weights, m.model = pf->model, m.model0 = pf->model0, m.hist = pf->hist, m.state = pf->state;
    return m;
}

// Three launches whatever count is; the frames go by value (a shared frame is repeated for every member).
int enqueue_group_tick(micv_pf_group *g, const uint8_t *const *frames, const size_t *strides, int nframes, hipStream_t s,
                       micv_pf_state *states_out) {
    GroupFrames f{};
    for (int k = 0; k < g->count; k++) {
        f.frame[k] = frames[nframes == 1 ? 0 : k];
        f.stride[k] = strides[nframes == 1 ? 0 : k];
    }
    pf_group_score_kernel<<<dim3(g->max_n, g->count), kScoreThreads, 0, s>>>(g->table, f);
    MICV_LAUNCH_CHECK();
    pf_group_resample_kernel<<<g->count, kTailThreads, 0, s>>>(g->table, states_out);
    MICV_LAUNCH_CHECK();
    pf_group_model_kernel<<<g->count, kTailThreads, 0, s>>>(g->table, f);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int group_frame_buffers(micv_pf_group *g) {
    for (auto &b : g->frame_buf)
        if (!b) MICV_HIP(hipMalloc(&b, g->frame_bytes()));
    return MICV_OK;
}

}  // namespace

// For ps6.hip (pf.hpp).
int pf_enqueue_tick(micv_pf *pf, const uint8_t *frame, size_t stride, hipStream_t s, micv_pf_state *state_out) {
    return enqueue_tick(pf, frame, stride, s, state_out);
}
int pf_frame_buffers(micv_pf *pf) { return frame_buffers(pf); }
int pf_group_enqueue_tick(micv_pf_group *g, const uint8_t *const *frames, const size_t *strides, int nframes, hipStream_t s,
                          micv_pf_state *states_out) {
    return enqueue_group_tick(g, frames, strides, nframes, s, states_out);
}
int pf_group_frame_buffers(micv_pf_group *g) { return group_frame_buffers(g); }

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

int micv_pf_group_create(micv_pf *const *members, int count, micv_pf_group **out) {
    MICV_REQUIRE(members && out, "micv_pf_group_create: null argument");
    *out = nullptr;
    MICV_REQUIRE(count >= 1 && count <= MICV_PF_GROUP_MAX, "micv_pf_group_create: count = %d outside 1 .. %d", count,
                 MICV_PF_GROUP_MAX);
    for (int k = 0; k < count; k++) {
        MICV_REQUIRE(members[k], "micv_pf_group_create: member %d is null", k);
        for (int j = 0; j < k; j++) MICV_REQUIRE(members[j] != members[k], "micv_pf_group_create: member %d is member %d", k, j);
        const micv_pf *a = members[0], *b = members[k];
        MICV_REQUIRE(b->device == a->device, "micv_pf_group_create: member %d lives on device %d, member 0 on %d", k, b->device,
                     a->device);
        MICV_REQUIRE(b->rows == a->rows && b->cols == a->cols && b->ch == a->ch,
                     "micv_pf_group_create: member %d was made for %d x %d x %d frames, member 0 for %d x %d x %d", k, b->rows,
                     b->cols, b->ch, a->rows, a->cols, a->ch);
    }
    std::unique_ptr<micv_pf_group> g(new micv_pf_group);
    g->device = members[0]->device, g->count = count;
    g->rows = members[0]->rows, g->cols = members[0]->cols, g->ch = members[0]->ch;
    g->members.assign(members, members + count);
    std::vector<PfMember> table(count);
    for (int k = 0; k < count; k++) {
        table[k] = describe(members[k]);
        g->max_n = std::max(g->max_n, members[k]->n);
    }
    MICV_HIP(hipSetDevice(g->device));
    MICV_HIP(hipMalloc(&g->table, count * sizeof(PfMember)));
    MICV_HIP(hipMemcpy(g->table, table.data(), count * sizeof(PfMember), hipMemcpyHostToDevice));
    *out = g.release();
    return MICV_OK;
}

void micv_pf_group_destroy(micv_pf_group *g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();  // nothing enqueued on its table or buffers may still run
    delete g;
}

int micv_pf_group_tick_dev(micv_pf_group *g, const uint8_t *const *frames, const size_t *strides, int nframes,
                           micv_stream stream, micv_pf_state *states_dev) {
    MICV_REQUIRE(g && frames && strides, "micv_pf_group_tick_dev: null argument");
    MICV_REQUIRE(nframes == 1 || nframes == g->count, "micv_pf_group_tick_dev: %d frames for %d members, need 1 or %d", nframes,
                 g->count, g->count);
    for (int k = 0; k < nframes; k++) {
        MICV_REQUIRE(frames[k], "micv_pf_group_tick_dev: frame %d is null", k);
        MICV_REQUIRE(strides[k] >= (size_t)g->cols * g->ch, "micv_pf_group_tick_dev: stride %zu of frame %d < %d", strides[k], k,
                     g->cols * g->ch);
    }
    MICV_HIP(hipSetDevice(g->device));
    return enqueue_group_tick(g, frames, strides, nframes, static_cast<hipStream_t>(stream), states_dev);
}

int micv_pf_group_track_seq_host(micv_pf_group *g, const uint8_t *const *frames, int nframes, size_t stride,
                                 micv_pf_state *states, float *const *particles) {
    MICV_REQUIRE(g && frames && states && nframes >= 1, "micv_pf_group_track_seq_host: bad argument");
    const size_t rb = (size_t)g->cols * g->ch;
    MICV_REQUIRE(stride >= rb, "micv_pf_group_track_seq_host: stride %zu < %zu", stride, rb);
    for (int t = 0; t < nframes; t++) MICV_REQUIRE(frames[t], "micv_pf_group_track_seq_host: frame %d is null", t);
    MICV_HIP(hipSetDevice(g->device));
    MICV_TRY(group_frame_buffers(g));
    const int count = g->count;
    struct Scope {  // released on every way out, after everything enqueued has finished
        hipStream_t up = nullptr, run = nullptr;
        std::vector<hipEvent_t> ev;
        std::vector<void *> mem;
        ~Scope() {
            for (hipStream_t s : {up, run})
                if (s) (void)hipStreamSynchronize(s);
            for (hipEvent_t e : ev) (void)hipEventDestroy(e);
            for (hipStream_t s : {up, run})
                if (s) (void)hipStreamDestroy(s);
            for (void *p : mem)
                if (p) (void)hipFree(p);
        }
    } sc;
    MICV_HIP(hipStreamCreateWithFlags(&sc.up, hipStreamNonBlocking));
    MICV_HIP(hipStreamCreateWithFlags(&sc.run, hipStreamNonBlocking));
    sc.mem.assign(1 + (size_t)count, nullptr);  // the states, then member k's particles of every tick
    MICV_HIP(hipMalloc(&sc.mem[0], (size_t)nframes * count * sizeof(micv_pf_state)));
    for (int k = 0; particles && k < count; k++)
        if (particles[k]) MICV_HIP(hipMalloc(&sc.mem[1 + k], (size_t)nframes * g->members[k]->n * sizeof(float2)));
    std::vector<hipEvent_t> ev_up(nframes), ev_tick(nframes);
    sc.ev.reserve(2 * (size_t)nframes);
    for (auto *v : {&ev_up, &ev_tick})
        for (auto &e : *v) {
            MICV_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            sc.ev.push_back(e);
        }
    micv_pf_state *dst = static_cast<micv_pf_state *>(sc.mem[0]);
    auto upload = [&](int t) -> int {
        if (t >= 2) MICV_HIP(hipStreamWaitEvent(sc.up, ev_tick[t - 2], 0));  // its buffer's last reader
        MICV_HIP(hipMemcpy2DAsync(g->frame_buf[t & 1], rb, frames[t], stride, rb, g->rows, hipMemcpyHostToDevice, sc.up));
        MICV_HIP(hipEventRecord(ev_up[t], sc.up));
        return MICV_OK;
    };
    MICV_TRY(upload(0));
    for (int t = 0; t < nframes; t++) {
        const uint8_t *buf = g->frame_buf[t & 1];
        MICV_HIP(hipStreamWaitEvent(sc.run, ev_up[t], 0));
        MICV_TRY(enqueue_group_tick(g, &buf, &rb, 1, sc.run, dst + (size_t)t * count));
        for (int k = 0; k < count; k++)
            if (sc.mem[1 + k]) {
                const size_t pbytes = (size_t)g->members[k]->n * sizeof(float2);
                MICV_HIP(hipMemcpyAsync(static_cast<char *>(sc.mem[1 + k]) + (size_t)t * pbytes, g->members[k]->parts, pbytes,
                                        hipMemcpyDeviceToDevice, sc.run));
            }
        MICV_HIP(hipEventRecord(ev_tick[t], sc.run));
        if (t + 1 < nframes) MICV_TRY(upload(t + 1));  // (a pageable copy holds this thread: tick t runs meanwhile)
    }
    MICV_HIP(hipMemcpyAsync(states, sc.mem[0], (size_t)nframes * count * sizeof(micv_pf_state), hipMemcpyDeviceToHost, sc.run));
    for (int k = 0; k < count; k++)
        if (sc.mem[1 + k])
            MICV_HIP(hipMemcpyAsync(particles[k], sc.mem[1 + k], (size_t)nframes * g->members[k]->n * sizeof(float2),
                                    hipMemcpyDeviceToHost, sc.run));
    MICV_HIP(hipStreamSynchronize(sc.run));
    return MICV_OK;
}

}  // extern "C"
