// mhi.hip -- ps7 motion-history path: frame differencing and the MHI
// update.  Byte kernels, HBM-bound by nature; the blur reuses the separable fmaf-chain contract.
//
//   mhi::frameDifference (MotionHistory.cpp:26-77), single-channel CV_8U frames:
//     Gaussian blur of both frames (cv::cuda separable filter: u8 -> float row pass -> column pass
//     -> saturate_cast<uchar>), saturating subtract f2 - f1, AbsThreshold -> {0,1}
//     (MotionHistory.cu:17-48), morphological OPEN with the 7x7 ellipse (erode, dilate; each pass
//     pads with BORDER_REFLECT_101 like cv::cuda's copyMakeBorder).
//   mhi::calcMotionHistory -> motionHistoryKernel (MotionHistory.cu:52-66).
#include <cmath>

#include "kernels.hpp"

namespace micv {

__device__ __forceinline__ uint8_t sat_u8_rn(float v) {
    const int r = __float2int_rn(v);  // round-half-even like saturate_cast<uchar>(float)
    return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

// ---- mhi::frameDifference on bit planes (r05) ----------------------------------------------------------------------
// Two launches, no float or byte temporaries in HBM (r04: four launches through an f32 plane pair and two byte planes,
// 0.072 ms at 1080p = 0.011 of the HBM roofline):
//   mhi_blur_diff_bits_kernel   both frames' Gaussian blur in one LDS tile (row pass of both frames -> LDS, column pass,
//                               saturate_cast<uchar>), saturating subtract, AbsThreshold; a wave is one 64-column row
//                               segment, so its BALLOT is the mask: one 64-bit word per (row, 64-column tile), 1/8 B
//                               per pixel instead of 9.
//   mhi_open7_bits_kernel       the 7x7 elliptical OPEN on those words: a wave owns 64 columns x 52 rows, lane = row, one
//                               128-bit register pair = the row with 6 columns either side; a horizontal erosion /
//                               dilation of half-width r is a shift-and-combine ladder (3 steps for r = 3), the vertical
//                               combination takes the neighbours' rows by wave shuffles -- no LDS, no barriers, 7 row
//                               terms per pass.  BORDER_REFLECT_101 (cv::cuda pads every pass): the mask is EXTENDED by
//                               reflection (rows: the lanes beyond the image load the reflected row; columns: edge tiles
//                               assemble their 76 bits one by one), and because the ellipse is symmetric in both axes the
//                               erosion of the extended mask IS the reflected extension of the eroded image, so the
//                               dilation's padding needs no second pass.
__global__ __launch_bounds__(256) void mhi_blur_diff_bits_kernel(const uint8_t *__restrict__ f1, const uint8_t *__restrict__ f2,
                                                                  size_t stride, int rows, int cols, Taps tx, Taps ty, double thresh,
                                                                  unsigned long long *__restrict__ words, int tiles_x) {
    constexpr int TW = 64, TH = 16;
    // dynamic LDS: the source tile of both frames as floats (every pixel converted once, the reflected border resolved
    // once), then the row-pass values of both frames
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int ax = tx.n / 2, ay = ty.n / 2, nrp = TH + 2 * ay, SW = TW + 2 * ax;
    float *S = sm, *RP = sm + 2 * nrp * SW;  // S[f][r][cx], RP[f][r][c]
    // the taps in LDS: a run-time index into the by-value Taps is a dependent scalar load per tap (measured: 22 us at
    // blur 5), 62 constant-index taps do not fit the scalar registers (62 spills, slower still)
    __shared__ float TX[32], TY[32];
    if (threadIdx.x < 32) {
        TX[threadIdx.x] = threadIdx.x < (unsigned)tx.n ? tx.k[threadIdx.x] : 0.f;
        TY[threadIdx.x] = threadIdx.x < (unsigned)ty.n ? ty.k[threadIdx.x] : 0.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // a wave stages whole rows (64 consecutive bytes per load), FOUR rows' loads in flight at a time: a load -> convert
    // -> ds_write loop serialises on every round trip (18 of them per wave at blur 3 = the whole launch time)
    const int c1 = reflect101(x0 - ax + lane, cols), c2 = reflect101(x0 - ax + lane + 64 < x0 + TW + ax ? x0 - ax + lane + 64 : x0, cols);
    const bool second = lane + 64 < SW;
    for (int j0 = wave; j0 < 2 * nrp; j0 += 16) {
        uint8_t va[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + 4 * u < 2 * nrp ? j0 + 4 * u : 2 * nrp - 1;
            const int f = j >= nrp, r = j - f * nrp;
            const uint8_t *s = (f ? f2 : f1) + (size_t)reflect101(y0 - ay + r, rows) * stride;
            va[u] = s[c1];
            vb[u] = s[c2];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + 4 * u;
            if (j < 2 * nrp) {
                S[j * SW + lane] = (float)va[u];
                if (second) S[j * SW + lane + 64] = (float)vb[u];
            }
        }
    }
    __syncthreads();
    const int c = lane, x = x0 + c;
    const int ntx = tx.n, nty = ty.n;
    for (int j = wave; j < 2 * nrp; j += 4) {
        const float *sp = S + j * SW + c;
        float acc = 0.f;
#pragma unroll 4
        for (int k = 0; k < ntx; k++) acc = fmaf(sp[k], TX[k], acc);
        RP[j * TW + c] = acc;
    }
    __syncthreads();
    // column pass, saturate, saturating subtract f2 - f1 (cv::cuda::subtract on CV_8U), AbsThreshold (MotionHistory.cu:17-48)
    for (int r = wave; r < TH; r += 4) {  // (wave-uniform)
        const int y = y0 + r;
        if (y >= rows) break;
        float a1 = 0.f, a2 = 0.f;
#pragma unroll 4
        for (int k = 0; k < nty; k++) {
            a1 = fmaf(RP[(r + k) * TW + c], TY[k], a1);
            a2 = fmaf(RP[(nrp + r + k) * TW + c], TY[k], a2);
        }
        const int d = (int)sat_u8_rn(a2) - (int)sat_u8_rn(a1);
        const int val = d < 0 ? 0 : d;
        const bool on = x < cols && ((double)val >= thresh || (double)(-val) >= thresh);
        const unsigned long long m = __ballot(on);
        if (c == 0) words[(size_t)y * tiles_x + blockIdx.x] = m;
    }
}

// ---- colour frames (CV_8UC3 / CV_8UC4, interleaved) and the body the video batch shares ---------------------------
// mhi::frameDifference on a cv::VideoCapture frame (MotionHistory.cpp:50-64): blur per channel, saturating subtract
// per channel, cvtColor(RGB2GRAY) of the DIFFERENCE, then threshold and open.  The channels go ONE AFTER ANOTHER
// through the LDS tile of the single-channel kernel (58 KB at 31 x 31: three copies side by side would cost a CU its
// second workgroup); each lane keeps the weighted sum of its four output rows in registers, and the per-row ballot at
// the end is the mask word as before.  Staged per channel: consecutive lanes read bytes `channels` apart (a wave's 64
// loads fall into 192 or 256 consecutive bytes, two to four 128-byte lines instead of one), which keeps the LDS tile
// and the row pass exactly those of one plane; staging the whole interleaved segment would need `channels` times the
// S rows in LDS or a second, byte-typed tile beside it.
// channels == 1 takes no weighting at all: the bytes of mhi_blur_diff_bits_kernel.
__device__ __forceinline__ void blur_diff_bits_c_body(const uint8_t *__restrict__ f1, const uint8_t *__restrict__ f2, size_t stride,
                                                      int rows, int cols, int channels, const Taps &tx, const Taps &ty, double thresh,
                                                      unsigned long long *__restrict__ words, int tiles_x, float *sm) {
    constexpr int TW = 64, TH = 16;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int ax = tx.n / 2, ay = ty.n / 2, nrp = TH + 2 * ay, SW = TW + 2 * ax;
    float *S = sm, *RP = sm + 2 * nrp * SW;  // S[f][r][cx], RP[f][r][c]: one channel at a time
    __shared__ float TX[32], TY[32];
    if (threadIdx.x < 32) {
        TX[threadIdx.x] = threadIdx.x < (unsigned)tx.n ? tx.k[threadIdx.x] : 0.f;
        TY[threadIdx.x] = threadIdx.x < (unsigned)ty.n ? ty.k[threadIdx.x] : 0.f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c1 = reflect101(x0 - ax + lane, cols), c2 = reflect101(x0 - ax + lane + 64 < x0 + TW + ax ? x0 - ax + lane + 64 : x0, cols);
    const bool second = lane + 64 < SW;
    const int c = lane, x = x0 + c;
    const int ntx = tx.n, nty = ty.n;
    const int nch = channels < 3 ? channels : 3;  // the 4th channel is never read
    int g[TH / 4] = {0, 0, 0, 0};                 // rows wave, wave + 4, wave + 8, wave + 12 of the tile
    for (int ch = 0; ch < nch; ch++) {
        // COLOR_RGB2GRAY's 8-bit weights in channel order (pyramid.hip: 4899, 9617, 1868 of 16384)
        const int wgt = nch == 1 ? 1 : (ch == 0 ? 4899 : (ch == 1 ? 9617 : 1868));
        const size_t o1 = (size_t)c1 * channels + ch, o2 = (size_t)c2 * channels + ch;
        // (the column pass of the previous channel read RP only; S is free since the barrier behind its row pass)
        for (int j0 = wave; j0 < 2 * nrp; j0 += 16) {
            uint8_t va[4], vb[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + 4 * u < 2 * nrp ? j0 + 4 * u : 2 * nrp - 1;
                const int f = j >= nrp, r = j - f * nrp;
                const uint8_t *s = (f ? f2 : f1) + (size_t)reflect101(y0 - ay + r, rows) * stride;
                va[u] = s[o1];
                vb[u] = s[o2];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = j0 + 4 * u;
                if (j < 2 * nrp) {
                    S[j * SW + lane] = (float)va[u];
                    if (second) S[j * SW + lane + 64] = (float)vb[u];
                }
            }
        }
        __syncthreads();  // (also: every wave has left the previous channel's column pass, so RP may be overwritten)
        for (int j = wave; j < 2 * nrp; j += 4) {
            const float *sp = S + j * SW + c;
            float acc = 0.f;
#pragma unroll 4
            for (int k = 0; k < ntx; k++) acc = fmaf(sp[k], TX[k], acc);
            RP[j * TW + c] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < TH / 4; i++) {
            const int r = wave + 4 * i;
            if (y0 + r < rows) {  // (wave-uniform; no break: the barriers of the next channel are still to come)
                float a1 = 0.f, a2 = 0.f;
#pragma unroll 4
                for (int k = 0; k < nty; k++) {
                    a1 = fmaf(RP[(r + k) * TW + c], TY[k], a1);
                    a2 = fmaf(RP[(nrp + r + k) * TW + c], TY[k], a2);
                }
                const int d = (int)sat_u8_rn(a2) - (int)sat_u8_rn(a1);
                g[i] += (d < 0 ? 0 : d) * wgt;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < TH / 4; i++) {
        const int y = y0 + wave + 4 * i;
        if (y < rows) {
            const int val = nch == 1 ? g[i] : (g[i] + 8192) >> 14;  // <= 255: the weights sum to 16384
            const bool on = x < cols && ((double)val >= thresh || (double)(-val) >= thresh);
            const unsigned long long m = __ballot(on);
            if (c == 0) words[(size_t)y * tiles_x + blockIdx.x] = m;
        }
    }
}

__global__ __launch_bounds__(256) void mhi_blur_diff_bits_c_kernel(const uint8_t *__restrict__ f1, const uint8_t *__restrict__ f2,
                                                                    size_t stride, int rows, int cols, int channels, Taps tx, Taps ty,
                                                                    double thresh, unsigned long long *__restrict__ words, int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    blur_diff_bits_c_body(f1, f2, stride, rows, cols, channels, tx, ty, thresh, words, tiles_x, sm);
}

// The per-video table of micv_mhi_history_batch_dev, by value in the kernarg block: one piece of a batch.
constexpr int kMhiBatchPiece = 32;
struct MhiBatchTable {
    const uint8_t *frames[kMhiBatchPiece];  // frame 0 of the video
    double thresh[kMhiBatchPiece];
    int save[kMhiBatchPiece];               // the video's last update
    int tau[kMhiBatchPiece];
};

// Step `step` of every video of the piece that still runs (blockIdx.z = video): frames step - 1 and step -> mask words.
__global__ __launch_bounds__(256) void mhi_blur_diff_bits_batch_kernel(MhiBatchTable t, int step, size_t frame_pitch, size_t stride,
                                                                        int rows, int cols, int channels, Taps tx, Taps ty,
                                                                        unsigned long long *__restrict__ words, size_t video_words,
                                                                        int tiles_x) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int v = blockIdx.z;
    if (step > t.save[v]) return;  // (block-uniform, before any barrier)
    const uint8_t *f1 = t.frames[v] + (size_t)(step - 1) * frame_pitch;
    blur_diff_bits_c_body(f1, f1 + frame_pitch, stride, rows, cols, channels, tx, ty, t.thresh[v], words + (size_t)v * video_words,
                          tiles_x, sm);
}

struct U128 {
    unsigned long long lo, hi;
};
__device__ __forceinline__ U128 u_and(U128 a, U128 b) { return {a.lo & b.lo, a.hi & b.hi}; }
__device__ __forceinline__ U128 u_or(U128 a, U128 b) { return {a.lo | b.lo, a.hi | b.hi}; }
template <int T>
__device__ __forceinline__ U128 u_shr(U128 a) { return {(a.lo >> T) | (a.hi << (64 - T)), a.hi >> T}; }  // bit k <- bit k + T
template <int T>
__device__ __forceinline__ U128 u_shl(U128 a) { return {a.lo << T, (a.hi << T) | (a.lo >> (64 - T))}; }  // bit k <- bit k - T
__device__ __forceinline__ U128 u_shfl(U128 a, int src_lane) {
    U128 r;
    r.lo = __shfl(a.lo, src_lane, 64);
    r.hi = __shfl(a.hi, src_lane, 64);
    return r;
}

// Horizontal pass of one ellipse row: bit k of H<r> = AND (OR) of bits k - r .. k + r.  The 7x7 ellipse of
// cv::getStructuringElement has rows of half-width 0, 2, 3, 3, 3, 2, 0 (ellipse7() below; checked by the host).
template <bool DILATE>
__device__ __forceinline__ void morph_rows(U128 e, U128 &h2, U128 &h3) {
    auto op = [](U128 a, U128 b) { return DILATE ? u_or(a, b) : u_and(a, b); };
    const U128 w2 = op(e, u_shr<1>(e));    // bits k, k + 1
    const U128 w4 = op(w2, u_shr<2>(w2));  // k .. k + 3
    const U128 w5 = op(w4, u_shr<1>(w4));  // k .. k + 4
    const U128 w7 = op(w4, u_shr<3>(w4));  // k .. k + 6
    h2 = u_shl<2>(w5);                     // centred: k - 2 .. k + 2
    h3 = u_shl<3>(w7);                     // k - 3 .. k + 3
}
// The vertical combination: row y of the result = rows y - 3 .. y + 3 through their ellipse rows.
template <bool DILATE>
__device__ __forceinline__ U128 morph7_bits(U128 e, int lane) {
    U128 h2, h3;
    morph_rows<DILATE>(e, h2, h3);
    auto op = [](U128 a, U128 b) { return DILATE ? u_or(a, b) : u_and(a, b); };
    U128 r = h3;
    r = op(r, u_shfl(h3, lane - 1));
    r = op(r, u_shfl(h3, lane + 1));
    r = op(r, u_shfl(h2, lane - 2));
    r = op(r, u_shfl(h2, lane + 2));
    r = op(r, u_shfl(e, lane - 3));
    r = op(r, u_shfl(e, lane + 3));
    return r;  // (lanes within 3 of the wave's ends hold wrapped rows: the caller uses the inner lanes only)
}

// The opened mask word of (row yb + lane - 6, word tx): valid in lanes 6 .. 57.
__device__ __forceinline__ unsigned long long open7_word(const unsigned long long *__restrict__ words, int tiles_x, int rows, int cols,
                                                         int tx, int yb, int lane) {
    const int x0 = 64 * tx;
    const int y = yb + lane - 6;
    const unsigned long long *row = words + (size_t)reflect101(y, rows) * tiles_x;
    // the row with 6 columns either side: bit k <-> column x0 - 6 + k, k = 0 .. 75
    U128 e;
    if (x0 - 6 >= 0 && x0 + 70 <= cols) {
        const unsigned long long cw = row[tx], lw = tx > 0 ? row[tx - 1] : 0ull, rw = x0 + 64 < cols ? row[tx + 1] : 0ull;
        e.lo = (lw >> 58) | (cw << 6);
        e.hi = ((cw >> 58) | (rw << 6)) & 0xFFFull;
    } else {
        // edge tiles: the columns outside the image by reflection (also the centre word's columns past a ragged right
        // edge).  Their sources lie in this tile or a neighbour: three words loaded up front, no memory in the loop.
        const int t0 = tx > 0 ? tx - 1 : 0, t2 = tx + 1 < tiles_x ? tx + 1 : tiles_x - 1;
        const unsigned long long w0 = row[t0], w1 = row[tx], w2 = row[t2];
        e.lo = ((tx > 0 ? w0 : 0ull) >> 58) | (w1 << 6);
        e.hi = ((w1 >> 58) | ((tx + 1 < tiles_x ? w2 : 0ull) << 6)) & 0xFFFull;
        const int k_lo_end = x0 - 6 < 0 ? 6 - x0 : 0;                       // columns < 0: k in [0, k_lo_end)
        const int k_hi_begin = cols - (x0 - 6) < 76 ? cols - (x0 - 6) : 76;  // columns >= cols: k in [k_hi_begin, 76)
        for (int k = 0; k < 76; k++) {
            if (k >= k_lo_end && k < k_hi_begin) continue;
            const int xx = reflect101(x0 - 6 + k, cols), tw = xx >> 6;
            const unsigned long long wsel = tw == tx ? w1 : (tw == t0 ? w0 : w2);
            const unsigned long long bit = (wsel >> (xx & 63)) & 1ull;
            if (k < 64) e.lo = (e.lo & ~(1ull << k)) | (bit << k);
            else e.hi = (e.hi & ~(1ull << (k - 64))) | (bit << (k - 64));
        }
    }
    const U128 er = morph7_bits<false>(e, lane);   // valid: lanes 3 .. 60, bits 3 .. 72
    const U128 op = morph7_bits<true>(er, lane);   // valid: lanes 6 .. 57, bits 6 .. 69
    return (op.lo >> 6) | (op.hi << 58);
}

__global__ __launch_bounds__(256) void mhi_open7_bits_kernel(const unsigned long long *__restrict__ words, int tiles_x, int rows,
                                                              int cols, uint8_t *__restrict__ dst, size_t dstride) {
    constexpr int OUT_ROWS = 52;  // 64 lanes = 52 output rows + 6 either side (3 for the erosion, 3 for the dilation)
    __shared__ unsigned long long W[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tx = blockIdx.x, x0 = 64 * tx;
    const int yb = (blockIdx.y * 4 + wave) * OUT_ROWS;
    if (yb >= rows) return;  // (wave-uniform; no workgroup barrier below)
    W[wave][lane] = open7_word(words, tiles_x, rows, cols, tx, yb, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // bytes out: four rows per wave-instruction, a lane expands four mask bits into one dword (64 contiguous bytes per row)
    const int d4 = lane & 15, rg = lane >> 4;
    for (int it = 0; it < OUT_ROWS / 4; it++) {
        const int r = 4 * it + rg, yo = yb + r;
        if (yo >= rows) continue;
        const unsigned bits = (unsigned)(W[wave][r + 6] >> (4 * d4)) & 0xFu;
        const unsigned bytes = (bits * 0x00204081u) & 0x01010101u;
        const int xo = x0 + 4 * d4;
        uint8_t *o = dst + (size_t)yo * dstride + xo;
        if (xo + 3 < cols && ((reinterpret_cast<uintptr_t>(o) & 3) == 0)) {
            *reinterpret_cast<unsigned *>(o) = bytes;
        } else {
            for (int b = 0; b < 4; b++)
                if (xo + b < cols) o[b] = (uint8_t)((bytes >> (8 * b)) & 1u);
        }
    }
}

// The open of step `step` with calcMotionHistory fused into its byte write (MotionHistory.cu:63-65:
// `bit ? tau : max(h - 1, 0)`, tau stored modulo 256): the history of video blockIdx.z is its output plane, which starts
// as zero -- step 1 does not read it -- and is not touched again once the video is past its save number.
__global__ __launch_bounds__(256) void mhi_open7_update_batch_kernel(MhiBatchTable t, int step, const unsigned long long *__restrict__ words,
                                                                      size_t video_words, int tiles_x, int rows, int cols,
                                                                      uint8_t *__restrict__ out, size_t out_pitch, size_t out_stride) {
    constexpr int OUT_ROWS = 52;
    __shared__ unsigned long long W[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = blockIdx.z;
    if (step > t.save[v]) return;  // (block-uniform)
    const int tx = blockIdx.x, x0 = 64 * tx;
    const int yb = (blockIdx.y * 4 + wave) * OUT_ROWS;
    if (yb >= rows) return;  // (wave-uniform; no workgroup barrier below)
    W[wave][lane] = open7_word(words + (size_t)v * video_words, tiles_x, rows, cols, tx, yb, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const unsigned tau8 = (unsigned)t.tau[v] & 0xFFu;
    uint8_t *hist = out + (size_t)v * out_pitch;
    const int d4 = lane & 15, rg = lane >> 4;
    for (int it = 0; it < OUT_ROWS / 4; it++) {
        const int r = 4 * it + rg, yo = yb + r;
        if (yo >= rows) continue;
        const unsigned bits = (unsigned)(W[wave][r + 6] >> (4 * d4)) & 0xFu;
        const int xo = x0 + 4 * d4;
        uint8_t *o = hist + (size_t)yo * out_stride + xo;
        if (xo + 3 < cols && ((reinterpret_cast<uintptr_t>(o) & 3) == 0)) {
            const unsigned h4 = step > 1 ? *reinterpret_cast<const unsigned *>(o) : 0u;
            unsigned res = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const unsigned h = (h4 >> (8 * b)) & 0xFFu;
                res |= (((bits >> b) & 1u) ? tau8 : (h ? h - 1 : 0u)) << (8 * b);
            }
            *reinterpret_cast<unsigned *>(o) = res;
        } else {
            for (int b = 0; b < 4; b++)
                if (xo + b < cols) {
                    const unsigned h = step > 1 ? o[b] : 0u;
                    o[b] = (uint8_t)(((bits >> b) & 1u) ? tau8 : (h ? h - 1 : 0u));
                }
        }
    }
}

// mhi::energyFromHistory (MotionHistory.cpp:98-105): any nonzero history value -> 1.
__global__ __launch_bounds__(256) void mhi_energy_kernel(const uint8_t *__restrict__ mhi, size_t sstride,
                                                          int rows, int cols, uint8_t *__restrict__ mei,
                                                          size_t dstride) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    mei[(size_t)y * dstride + x] = mhi[(size_t)y * sstride + x] > 0 ? 1 : 0;
}

struct Ellipse7 {
    unsigned char m[7];  // bit j of m[i] = element (i, j)
};

__global__ __launch_bounds__(256) void mhi_threshold_kernel(const uint8_t *__restrict__ src,
                                                             size_t sstride, int rows, int cols,
                                                             double thresh,
                                                             uint8_t *__restrict__ dst,
                                                             size_t dstride) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    const int val = src[(size_t)y * sstride + x];
    dst[(size_t)y * dstride + x] = ((double)val >= thresh || (double)(-val) >= thresh) ? 1 : 0;
}

__global__ __launch_bounds__(256) void mhi_update_kernel(uint8_t *__restrict__ hist, size_t hstride,
                                                          const uint8_t *__restrict__ mask,
                                                          size_t mstride, int rows, int cols,
                                                          int tau) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    const int h = hist[(size_t)y * hstride + x];
    hist[(size_t)y * hstride + x] =
        (uint8_t)(mask[(size_t)y * mstride + x] == 1 ? tau : (h - 1 > 0 ? h - 1 : 0));  // MotionHistory.cu:63-65
}

// cv::getStructuringElement(MORPH_ELLIPSE, Size(7,7)).
static Ellipse7 ellipse7() {
    Ellipse7 e;
    const int r = 3, c = 3;
    const double inv_r2 = 1.0 / ((double)r * r);
    for (int i = 0; i < 7; i++) {
        const int dy = i - r;
        const int dx = (int)std::lrint(c * std::sqrt((r * r - dy * dy) * inv_r2));
        const int j1 = c - dx < 0 ? 0 : c - dx, j2 = c + dx + 1 > 7 ? 7 : c + dx + 1;
        e.m[i] = 0;
        for (int j = j1; j < j2; j++) e.m[i] |= (unsigned char)(1u << j);
    }
    return e;
}

// The scratch micv_mhi_frame_difference_dev carves from the start of the context arena (its bit-plane words).
// micv_mhi_history_seq_dev keeps its own planes after this many bytes, so both take the size from here.
static size_t frame_difference_scratch(int rows, int cols) { return Carver::need((size_t)rows * cdiv(cols, 64), 8); }

// Dynamic LDS of the blur kernels: S and RP of both frames, one channel (<= 58 KB at 31 x 31).
static size_t blur_tile_lds(int blur_w, int blur_h) {
    return (size_t)2 * (16 + 2 * (blur_h / 2)) * (64 + 2 * (blur_w / 2) + 64) * sizeof(float);
}

// the bit-plane open is written for the 7x7 ellipse's row half-widths 0, 2, 3, 3, 3, 2, 0
static int check_ellipse7(const char *fn) {
    const Ellipse7 e = ellipse7();
    static const unsigned char want[7] = {0x08, 0x3E, 0x7F, 0x7F, 0x7F, 0x3E, 0x08};
    for (int i = 0; i < 7; i++)
        if (e.m[i] != want[i]) {
            set_error("%s: unexpected 7x7 ellipse row %d = %#x", fn, i, e.m[i]);
            return MICV_EUNSUPPORTED;
        }
    return MICV_OK;
}

}  // namespace micv

using namespace micv;

extern "C" {

int micv_mhi_frame_difference_dev(micv_ctx *ctx, const uint8_t *f1, const uint8_t *f2, int rows,
                                  int cols, size_t stride, double thresh, int blur_w, int blur_h,
                                  double blur_sigma, uint8_t *diff, size_t dstride,
                                  micv_stream stream) {
    MICV_REQUIRE(ctx && f1 && f2 && diff, "micv_mhi_frame_difference: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && stride >= (size_t)cols && dstride >= (size_t)cols,
                 "micv_mhi_frame_difference: bad size / stride");
    MICV_REQUIRE(blur_w >= 1 && blur_w <= 31 && (blur_w & 1) && blur_h >= 1 && blur_h <= 31 && (blur_h & 1) &&
                     blur_sigma > 0,
                 "micv_mhi_frame_difference: blur %dx%d / sigma %g not supported (odd sizes <= 31, sigma > 0)",
                 blur_w, blur_h, blur_sigma);
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int tiles_x = cdiv(cols, 64);
    void *scratch;
    MICV_TRY(ctx->reserve(frame_difference_scratch(rows, cols), &scratch));
    unsigned long long *words = static_cast<unsigned long long *>(scratch);
    Taps t, ty;  // cv::Size(width, height): width taps along x, height taps along y
    gaussian_taps(blur_w, blur_sigma, &t);
    gaussian_taps(blur_h, blur_sigma, &ty);
    MICV_TRY(check_ellipse7("micv_mhi_frame_difference"));
    const size_t lds = blur_tile_lds(blur_w, blur_h);
    mhi_blur_diff_bits_kernel<<<dim3(tiles_x, cdiv(rows, 16)), 256, lds, s>>>(f1, f2, stride, rows, cols, t, ty, thresh, words, tiles_x);
    MICV_LAUNCH_CHECK();
    mhi_open7_bits_kernel<<<dim3(tiles_x, cdiv(cdiv(rows, 52), 4)), 256, 0, s>>>(words, tiles_x, rows, cols, diff, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

// Colour frames: one launch in front of the open, as above; nothing but the mask words goes to HBM.
int micv_mhi_frame_difference_c_dev(micv_ctx *ctx, const uint8_t *f1, const uint8_t *f2, int rows, int cols, int channels,
                                    size_t stride, double thresh, int blur_w, int blur_h, double blur_sigma, uint8_t *diff,
                                    size_t dstride, micv_stream stream) {
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_mhi_frame_difference_c: channels %d (1, 3 or 4)", channels);
    if (channels == 1)
        return micv_mhi_frame_difference_dev(ctx, f1, f2, rows, cols, stride, thresh, blur_w, blur_h, blur_sigma, diff, dstride, stream);
    MICV_REQUIRE(ctx && f1 && f2 && diff, "micv_mhi_frame_difference_c: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0, "micv_mhi_frame_difference_c: bad size %d x %d", rows, cols);
    MICV_REQUIRE(stride >= (size_t)cols * channels, "micv_mhi_frame_difference_c: stride %zu < cols * channels = %zu", stride,
                 (size_t)cols * channels);
    MICV_REQUIRE(dstride >= (size_t)cols, "micv_mhi_frame_difference_c: dstride %zu < cols", dstride);
    MICV_REQUIRE(blur_w >= 1 && blur_w <= 31 && (blur_w & 1) && blur_h >= 1 && blur_h <= 31 && (blur_h & 1) &&
                     blur_sigma > 0,
                 "micv_mhi_frame_difference_c: blur %dx%d / sigma %g not supported (odd sizes <= 31, sigma > 0)",
                 blur_w, blur_h, blur_sigma);
    MICV_TRY(check_ellipse7("micv_mhi_frame_difference_c"));
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int tiles_x = cdiv(cols, 64);
    void *scratch;
    MICV_TRY(ctx->reserve(frame_difference_scratch(rows, cols), &scratch));
    unsigned long long *words = static_cast<unsigned long long *>(scratch);
    Taps t, ty;
    gaussian_taps(blur_w, blur_sigma, &t);
    gaussian_taps(blur_h, blur_sigma, &ty);
    mhi_blur_diff_bits_c_kernel<<<dim3(tiles_x, cdiv(rows, 16)), 256, blur_tile_lds(blur_w, blur_h), s>>>(
        f1, f2, stride, rows, cols, channels, t, ty, thresh, words, tiles_x);
    MICV_LAUNCH_CHECK();
    mhi_open7_bits_kernel<<<dim3(tiles_x, cdiv(cdiv(rows, 52), 4)), 256, 0, s>>>(words, tiles_x, rows, cols, diff, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_mhi_energy_dev(micv_ctx *ctx, const uint8_t *mhi, int rows, int cols, size_t sstride,
                        uint8_t *mei, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && mhi && mei, "micv_mhi_energy: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && sstride >= (size_t)cols && dstride >= (size_t)cols,
                 "micv_mhi_energy: bad size / stride");
    MICV_HIP(hipSetDevice(ctx->device));
    mhi_energy_kernel<<<dim3(cdiv(cols, 64), cdiv(rows, 4)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        mhi, sstride, rows, cols, mei, dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_mhi_threshold_dev(micv_ctx *ctx, const uint8_t *src, int rows, int cols, size_t sstride,
                           double thresh, uint8_t *dst, size_t dstride, micv_stream stream) {
    MICV_REQUIRE(ctx && src && dst, "micv_mhi_threshold: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && sstride >= (size_t)cols && dstride >= (size_t)cols,
                 "micv_mhi_threshold: bad size / stride");
    MICV_HIP(hipSetDevice(ctx->device));
    mhi_threshold_kernel<<<dim3(cdiv(cols, 64), cdiv(rows, 4)), 256, 0,
                           static_cast<hipStream_t>(stream)>>>(src, sstride, rows, cols, thresh, dst,
                                                               dstride);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}

int micv_mhi_update_dev(micv_ctx *ctx, uint8_t *history, size_t hstride, const uint8_t *mask,
                        size_t mstride, int rows, int cols, int tau, micv_stream stream) {
    MICV_REQUIRE(ctx && history && mask, "micv_mhi_update: null argument");
    MICV_REQUIRE(rows > 0 && cols > 0 && hstride >= (size_t)cols && mstride >= (size_t)cols,
                 "micv_mhi_update: bad size / stride");
    MICV_REQUIRE(tau > 0, "micv_mhi_update: tau must be > 0");  // MotionHistory.cpp:80
    MICV_HIP(hipSetDevice(ctx->device));
    mhi_update_kernel<<<dim3(cdiv(cols, 64), cdiv(rows, 4)), 256, 0, static_cast<hipStream_t>(stream)>>>(
        history, hstride, mask, mstride, rows, cols, tau);
    MICV_LAUNCH_CHECK();
    return MICV_OK;
}


// mhiHelper's loop (Solution.cpp:16-101): the history and difference planes sit in the scratch after
// frame_difference_scratch() bytes, the part frameDifference carves from its start; reserving the whole block first
// keeps frameDifference's own reserve() from moving them.
int micv_mhi_history_seq_dev(micv_ctx *ctx, const uint8_t *frames, int nframes, size_t frame_pitch, size_t stride,
                             int rows, int cols, double thresh, int blur_w, int blur_h, double blur_sigma, int tau,
                             const int *save, int nsave, uint8_t *out, size_t out_pitch, size_t out_stride,
                             micv_stream stream) {
    MICV_REQUIRE(ctx && frames && save && out, "micv_mhi_history_seq: null argument");
    MICV_REQUIRE(nframes >= 2 && nsave >= 1, "micv_mhi_history_seq: need >= 2 frames and >= 1 save number");
    MICV_REQUIRE(rows > 0 && cols > 0 && stride >= (size_t)cols && out_stride >= (size_t)cols &&
                     frame_pitch >= stride * (size_t)rows && (nsave == 1 || out_pitch >= out_stride * (size_t)rows),
                 "micv_mhi_history_seq: bad size / stride / pitch");
    MICV_REQUIRE(tau > 0, "micv_mhi_history_seq: tau must be > 0");
    MICV_REQUIRE(blur_w >= 1 && blur_w <= 31 && (blur_w & 1) && blur_h >= 1 && blur_h <= 31 && (blur_h & 1) &&
                     blur_sigma > 0,
                 "micv_mhi_history_seq: blur %dx%d / sigma %g not supported (odd sizes <= 31, sigma > 0)", blur_w,
                 blur_h, blur_sigma);
    int last = 0;
    for (int i = 0; i < nsave; i++) {
        MICV_REQUIRE(save[i] >= 1 && save[i] <= nframes - 1, "micv_mhi_history_seq: save number %d outside 1..%d",
                     save[i], nframes - 1);
        last = save[i] > last ? save[i] : last;
    }
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t words = frame_difference_scratch(rows, cols), plane = Carver::need((size_t)rows * cols, 1);
    void *scratch;
    MICV_TRY(ctx->reserve(words + 2 * plane, &scratch));
    uint8_t *hist = static_cast<uint8_t *>(scratch) + words, *diff = hist + plane;
    MICV_HIP(hipMemsetAsync(hist, 0, (size_t)rows * cols, s));
    for (int f = 1; f <= last; f++) {
        MICV_TRY(micv_mhi_frame_difference_dev(ctx, frames + (size_t)(f - 1) * frame_pitch, frames + (size_t)f * frame_pitch,
                                               rows, cols, stride, thresh, blur_w, blur_h, blur_sigma, diff, cols, stream));
        MICV_TRY(micv_mhi_update_dev(ctx, hist, cols, diff, cols, rows, cols, tau, stream));
        for (int i = 0; i < nsave; i++)
            if (save[i] == f)
                MICV_HIP(hipMemcpy2DAsync(out + (size_t)i * out_pitch, out_stride, hist, cols, cols, rows,
                                          hipMemcpyDeviceToDevice, s));
    }
    return MICV_OK;
}

// mhiHelper's loop with its two save lists (saveDiffFrames, saveMHIFrames) on frames of 1, 3 or 4 channels.
int micv_mhi_history_seq_c_dev(micv_ctx *ctx, const uint8_t *frames, int nframes, size_t frame_pitch, size_t stride, int rows,
                               int cols, int channels, double thresh, int blur_w, int blur_h, double blur_sigma, int tau,
                               const int *save, int nsave, uint8_t *out, size_t out_pitch, size_t out_stride,
                               const int *save_diff, int nsave_diff, uint8_t *diff_out, size_t diff_pitch, size_t diff_stride,
                               micv_stream stream) {
    MICV_REQUIRE(ctx && frames, "micv_mhi_history_seq_c: null argument");
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_mhi_history_seq_c: channels %d (1, 3 or 4)", channels);
    MICV_REQUIRE(nsave >= 0 && nsave_diff >= 0 && nsave + nsave_diff >= 1, "micv_mhi_history_seq_c: need >= 1 save number (nsave %d, nsave_diff %d)",
                 nsave, nsave_diff);
    MICV_REQUIRE((nsave == 0 || (save && out)) && (nsave_diff == 0 || (save_diff && diff_out)),
                 "micv_mhi_history_seq_c: a save list without its numbers or its output");
    MICV_REQUIRE(nframes >= 2, "micv_mhi_history_seq_c: nframes %d (need >= 2)", nframes);
    MICV_REQUIRE(rows > 0 && cols > 0, "micv_mhi_history_seq_c: bad size %d x %d", rows, cols);
    MICV_REQUIRE(stride >= (size_t)cols * channels, "micv_mhi_history_seq_c: stride %zu < cols * channels = %zu", stride,
                 (size_t)cols * channels);
    MICV_REQUIRE(frame_pitch >= stride * (size_t)rows, "micv_mhi_history_seq_c: frame_pitch %zu < stride * rows", frame_pitch);
    MICV_REQUIRE(nsave == 0 || (out_stride >= (size_t)cols && (nsave == 1 || out_pitch >= out_stride * (size_t)rows)),
                 "micv_mhi_history_seq_c: bad out_stride / out_pitch");
    MICV_REQUIRE(nsave_diff == 0 || (diff_stride >= (size_t)cols && (nsave_diff == 1 || diff_pitch >= diff_stride * (size_t)rows)),
                 "micv_mhi_history_seq_c: bad diff_stride / diff_pitch");
    MICV_REQUIRE(tau > 0, "micv_mhi_history_seq_c: tau must be > 0");
    MICV_REQUIRE(blur_w >= 1 && blur_w <= 31 && (blur_w & 1) && blur_h >= 1 && blur_h <= 31 && (blur_h & 1) &&
                     blur_sigma > 0,
                 "micv_mhi_history_seq_c: blur %dx%d / sigma %g not supported (odd sizes <= 31, sigma > 0)", blur_w,
                 blur_h, blur_sigma);
    int last = 0;
    for (int i = 0; i < nsave; i++) {
        MICV_REQUIRE(save[i] >= 1 && save[i] <= nframes - 1, "micv_mhi_history_seq_c: save number %d outside 1..%d",
                     save[i], nframes - 1);
        last = save[i] > last ? save[i] : last;
    }
    for (int i = 0; i < nsave_diff; i++) {
        MICV_REQUIRE(save_diff[i] >= 1 && save_diff[i] <= nframes - 1, "micv_mhi_history_seq_c: save_diff number %d outside 1..%d",
                     save_diff[i], nframes - 1);
        last = save_diff[i] > last ? save_diff[i] : last;
    }
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t words = frame_difference_scratch(rows, cols), plane = Carver::need((size_t)rows * cols, 1);
    void *scratch;
    MICV_TRY(ctx->reserve(words + 2 * plane, &scratch));
    uint8_t *hist = static_cast<uint8_t *>(scratch) + words, *diff = hist + plane;
    MICV_HIP(hipMemsetAsync(hist, 0, (size_t)rows * cols, s));
    for (int f = 1; f <= last; f++) {
        MICV_TRY(micv_mhi_frame_difference_c_dev(ctx, frames + (size_t)(f - 1) * frame_pitch, frames + (size_t)f * frame_pitch,
                                                 rows, cols, channels, stride, thresh, blur_w, blur_h, blur_sigma, diff, cols, stream));
        MICV_TRY(micv_mhi_update_dev(ctx, hist, cols, diff, cols, rows, cols, tau, stream));
        for (int i = 0; i < nsave; i++)
            if (save[i] == f)
                MICV_HIP(hipMemcpy2DAsync(out + (size_t)i * out_pitch, out_stride, hist, cols, cols, rows,
                                          hipMemcpyDeviceToDevice, s));
        for (int i = 0; i < nsave_diff; i++)
            if (save_diff[i] == f)
                MICV_HIP(hipMemcpy2DAsync(diff_out + (size_t)i * diff_pitch, diff_stride, diff, cols, cols, rows,
                                          hipMemcpyDeviceToDevice, s));
    }
    return MICV_OK;
}

constexpr size_t kMhiBatchBytes = size_t(64) << 20;  // the mask words of one piece of a batch stay below this

// getAllMHIs' loop (Solution.cpp:113-146) for V videos at once: step j is two launches over every video with save[v] >= j.
int micv_mhi_history_batch_dev(micv_ctx *ctx, const uint8_t *const *frames, const int *nframes, size_t frame_pitch, size_t stride,
                               int nvideos, int rows, int cols, int channels, const double *thresh, const int *tau, const int *save,
                               int blur_w, int blur_h, double blur_sigma, uint8_t *out, size_t out_pitch, size_t out_stride,
                               micv_stream stream) {
    MICV_REQUIRE(nvideos >= 1, "micv_mhi_history_batch: nvideos %d (need >= 1)", nvideos);
    MICV_REQUIRE(ctx && frames && nframes && thresh && tau && save && out, "micv_mhi_history_batch: null argument");
    MICV_REQUIRE(channels == 1 || channels == 3 || channels == 4, "micv_mhi_history_batch: channels %d (1, 3 or 4)", channels);
    MICV_REQUIRE(rows > 0 && cols > 0, "micv_mhi_history_batch: bad size %d x %d", rows, cols);
    MICV_REQUIRE(stride >= (size_t)cols * channels, "micv_mhi_history_batch: stride %zu < cols * channels = %zu", stride,
                 (size_t)cols * channels);
    MICV_REQUIRE(frame_pitch >= stride * (size_t)rows, "micv_mhi_history_batch: frame_pitch %zu < stride * rows", frame_pitch);
    MICV_REQUIRE(out_stride >= (size_t)cols && (nvideos == 1 || out_pitch >= out_stride * (size_t)rows),
                 "micv_mhi_history_batch: bad out_stride / out_pitch");
    MICV_REQUIRE(blur_w >= 1 && blur_w <= 31 && (blur_w & 1) && blur_h >= 1 && blur_h <= 31 && (blur_h & 1) &&
                     blur_sigma > 0,
                 "micv_mhi_history_batch: blur %dx%d / sigma %g not supported (odd sizes <= 31, sigma > 0)", blur_w,
                 blur_h, blur_sigma);
    for (int v = 0; v < nvideos; v++) {
        MICV_REQUIRE(frames[v], "micv_mhi_history_batch: frames[%d] is null", v);
        MICV_REQUIRE(nframes[v] >= 2, "micv_mhi_history_batch: nframes[%d] = %d (need >= 2)", v, nframes[v]);
        MICV_REQUIRE(tau[v] > 0, "micv_mhi_history_batch: tau[%d] must be > 0", v);
        MICV_REQUIRE(save[v] >= 1 && save[v] <= nframes[v] - 1, "micv_mhi_history_batch: save[%d] = %d outside 1..%d", v, save[v],
                     nframes[v] - 1);
    }
    MICV_TRY(check_ellipse7("micv_mhi_history_batch"));
    MICV_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int tiles_x = cdiv(cols, 64);
    // Pieces: at most kMhiBatchPiece videos (the by-value table) and as many as keep the mask words within the bound
    const size_t video_bytes = frame_difference_scratch(rows, cols), video_words = video_bytes / 8;
    size_t piece = kMhiBatchBytes / video_bytes < 1 ? 1 : kMhiBatchBytes / video_bytes;
    if (piece > (size_t)kMhiBatchPiece) piece = kMhiBatchPiece;
    if (piece > (size_t)nvideos) piece = nvideos;
    void *scratch;
    MICV_TRY(ctx->reserve(piece * video_bytes, &scratch));
    unsigned long long *words = static_cast<unsigned long long *>(scratch);
    Taps t, ty;
    gaussian_taps(blur_w, blur_sigma, &t);
    gaussian_taps(blur_h, blur_sigma, &ty);
    const size_t lds = blur_tile_lds(blur_w, blur_h);
    for (int v0 = 0; v0 < nvideos; v0 += (int)piece) {
        const int n = nvideos - v0 < (int)piece ? nvideos - v0 : (int)piece;
        MhiBatchTable tab = {};
        int last = 0;
        for (int i = 0; i < n; i++) {
            tab.frames[i] = frames[v0 + i];
            tab.thresh[i] = thresh[v0 + i];
            tab.save[i] = save[v0 + i];
            tab.tau[i] = tau[v0 + i];
            last = save[v0 + i] > last ? save[v0 + i] : last;
        }
        for (int j = 1; j <= last; j++) {
            mhi_blur_diff_bits_batch_kernel<<<dim3(tiles_x, cdiv(rows, 16), n), 256, lds, s>>>(
                tab, j, frame_pitch, stride, rows, cols, channels, t, ty, words, video_words, tiles_x);
            MICV_LAUNCH_CHECK();
            mhi_open7_update_batch_kernel<<<dim3(tiles_x, cdiv(cdiv(rows, 52), 4), n), 256, 0, s>>>(
                tab, j, words, video_words, tiles_x, rows, cols, out + (size_t)v0 * out_pitch, out_pitch, out_stride);
            MICV_LAUNCH_CHECK();
        }
    }
    return MICV_OK;
}

}  // extern "C"
