// The body of the score kernels (ransac.hip: one solve; ransac_pairs.hip: blockIdx.y = pair), included as text so that both
// compile from one source and the single-solve kernels keep the code they had.  In scope: kLds, pts, ctl, samples, seed,
// iters, type, smax, min_ratio, counts -- for the pair kernels those of ITS pair.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int n = ctl[0];
    const int k = type;
    if (n < k || ctl[2]) return;
    const float4 *P = pts;
    if (kLds) {
        float4 *lp = reinterpret_cast<float4 *>(smem);
        for (int j = threadIdx.x; j < n; j += blockDim.x) lp[j] = pts[j];
        __syncthreads();
        P = lp;
    }
    unsigned *stop = reinterpret_cast<unsigned *>(&ctl[1]);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t h0 = (int64_t)blockIdx.x * kChunk; h0 < iters; h0 += (int64_t)gridDim.x * kChunk) {
        // chunks ascend: once one starts after a known stop, so does every later one
        if ((uint64_t)h0 > __hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        const int hend = (int)std::min<int64_t>(h0 + kChunk, iters);
        for (int h = (int)h0 + wave; h < hend; h += kWaves) {
            int s[3];
            if (!draw_sample(samples, seed, h, k, n, s)) {
                if (lane == 0) {
                    atomicOr(&ctl[2], 1);
                    counts[h] = 0;
                }
                continue;
            }
            float4 q[3];
            for (int e = 0; e < 3; e++) q[e] = e < k ? P[s[e]] : make_float4(0.f, 0.f, 0.f, 0.f);
            float t[6];
            hypothesis(type, q, t);
            int cnt = 0;
            for (int j0 = 0; j0 < n; j0 += 64) {
                const int j = j0 + lane;
                const bool in = j < n && j != s[0] && j != s[1] && j != s[2] && point_pass(t, P[j], smax);
                cnt += __popcll(__ballot(in));
            }
            if (lane == 0) {
                counts[h] = cnt;
                if ((double)cnt / (double)n >= min_ratio) atomicMin(stop, (unsigned)h);
            }
        }
    }
