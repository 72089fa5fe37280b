// The body of the model kernels (pf.hip: pf_model_kernel; pf_group_model_kernel, member blockIdx.x), included as text for the
// reason pf_score_body.hpp gives.  updateModel at the rounded estimate: one workgroup of kTailThreads.
// In scope: frame, stride, rows, cols, ch, mrows, mcols, mode, fa, fb, state, model0, model, mhist -- for the group kernel
// those of ITS member.
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
