// The body of the score kernels (pf.hip: pf_score_kernel, particle blockIdx.x of one filter; pf_group_score_kernel, of member
// blockIdx.y), included as text so that both compile from one source and the single tick's kernel keeps the code it had: as
// an inline function the stage changed that kernel's register allocation (profiles/pf_group/resources.txt).
// Displace particle i (one workgroup of kScoreThreads), test it, score its patch: moved[i], sim[i] (0 outside the frame).
// In scope: i, frame, stride, rows, cols, ch, mrows, mcols, mode, flags, mse_sigma, parts, disp, model, mhist, moved, sim --
// for the group kernel those of ITS member.
    __shared__ unsigned bins[kScoreThreads / 64][3 * kBins];
    __shared__ unsigned long long red[kScoreThreads / 64];
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
