// The body of the finalize kernels, included as text like ransac_score_body.hpp.  In scope: pts, ctl, samples, seed, iters, type,
// smax, min_ratio, counts, transforms, mask, mask_len, stats -- for the pair kernel those of ITS pair.
    __shared__ unsigned first;
    __shared__ unsigned long long best_key;
    __shared__ float tb[6];
    __shared__ int sb[3];
    __shared__ int ran;  // 1: iterations ran, 0: none, -1: bad input
    const int n = ctl[0];
    const int k = type;
    if (threadIdx.x == 0) {
        first = ~0u;
        best_key = 0;
        ran = ctl[2] ? -1 : (n < k || 0.0 >= min_ratio) ? 0 : 1;
    }
    __syncthreads();
    if (ran != 1) {
        if (threadIdx.x == 0) {
            stats[0] = ran;
            stats[1] = -1;
            stats[2] = 0;
        }
        if (threadIdx.x < 12) transforms[threadIdx.x] = 0.f;
        for (int64_t j = threadIdx.x; j < mask_len; j += blockDim.x) mask[j] = 0;
        return;
    }
    // the stop iteration: the first i with count_i / n >= min_ratio.  Every i up to the stop word
    // was scored (and no i beyond it is read).
    const unsigned sw = (unsigned)ctl[1];
    const int bound = sw < (unsigned)iters ? (int)sw : iters - 1;
    unsigned f = ~0u;
    for (int i = threadIdx.x; i <= bound; i += blockDim.x)
        if ((double)counts[i] / (double)n >= min_ratio) {
            f = (unsigned)i;
            break;
        }
    atomicMin(&first, f);
    __syncthreads();
    const int last = first != ~0u ? (int)first : iters - 1;
    // the first maximum over [0, last]: the reference's strict '>' update
    unsigned long long key = 0;
    for (int i = threadIdx.x; i <= last; i += blockDim.x) {
        const unsigned long long kk = ((unsigned long long)(unsigned)counts[i] << 32) | (0xFFFFFFFFu - (unsigned)i);
        key = kk > key ? kk : key;
    }
    atomicMax(&best_key, key);
    __syncthreads();
    const int best = (int)(0xFFFFFFFFu - (unsigned)(best_key & 0xFFFFFFFFu));
    if (threadIdx.x == 0) {
        int s[3];
        float4 q[3];
        float t[6];
        draw_sample(samples, seed, last, k, n, s);
        for (int e = 0; e < 3; e++) q[e] = e < k ? pts[s[e]] : make_float4(0.f, 0.f, 0.f, 0.f);
        hypothesis(type, q, t);
        for (int e = 0; e < 6; e++) transforms[e] = t[e];
        draw_sample(samples, seed, best, k, n, s);
        for (int e = 0; e < 3; e++) q[e] = e < k ? pts[s[e]] : make_float4(0.f, 0.f, 0.f, 0.f);
        hypothesis(type, q, t);
        for (int e = 0; e < 6; e++) {
            transforms[6 + e] = t[e];
            tb[e] = t[e];
        }
        for (int e = 0; e < 3; e++) sb[e] = s[e];
        stats[0] = last + 1;
        stats[1] = best;
        stats[2] = (int)(best_key >> 32);
    }
    __syncthreads();
    float t[6];
    for (int e = 0; e < 6; e++) t[e] = tb[e];
    for (int64_t j = threadIdx.x; j < mask_len; j += blockDim.x)
        mask[j] = j < n && j != sb[0] && j != sb[1] && j != sb[2] && point_pass(t, pts[j], smax);
