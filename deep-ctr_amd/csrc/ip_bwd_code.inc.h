// ip_bwd_code.inc.h -- the code of k_ip_bwd<WV> (ip_gather_kernels.hip.h), included inside the solo kernel and inside its group form
// k_ip_bwd_g (ip_group_kernels.hip.h): `a` (IpBwdArgs), `dz`, `gxp` and `gb_part` are the including function's.  Text, not a __device__ function: as a
// function inlined into both kernels it compiled the solo kernel to other instructions than its own code in place does, and the
// solo step measured 0.7 % slower ("A mini-batch step for many inner-product models").
    extern __shared__ __align__(16) unsigned char smem[];
    float* se = reinterpret_cast<float*>(smem);                 // [16][F*16]
    float* sd = se + 16 * a.F * SLOT;                           // [16][D0p]
    float* sw = sd + 16 * a.D0p;                                // [16][F] value weights (WV only)
    const int tid = threadIdx.x, t0 = blockIdx.x * 16, F = a.F, K = a.K, B = a.B, FS = F * SLOT;
    const int P = a.P, CB = FS + P;
    // both tiles are contiguous in memory (16 consecutive rows): 16-byte pieces, eight loads in flight per thread before the
    // first LDS store (a copy loop of one load -> one store per trip pays one memory round trip per trip)
    auto fill = [&](float* dst, const float* __restrict__ src, const int n4) {
        for (int e0 = tid; e0 < n4; e0 += 256 * 8) {
            float4 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { const int e = e0 + 256 * k; v[k] = e < n4 ? *reinterpret_cast<const float4*>(src + 4 * (size_t)e) : make_float4(0.f, 0.f, 0.f, 0.f); }
#pragma unroll
            for (int k = 0; k < 8; ++k) { const int e = e0 + 256 * k; if (e < n4) *reinterpret_cast<float4*>(dst + 4 * e) = v[k]; }
        }
    };
    if (a.emb) fill(se, a.emb + (size_t)t0 * FS, 16 * FS / 4);       // the raw embeddings the forward gathered
    else ip_gather16<SLOT, 256, WV>(se, a.ids, a.table16, a.n_rows, t0, B, F, nullptr, a.wts);
    if (WV) for (int e = tid; e < 16 * F; e += 256) sw[e] = t0 + e / F < B ? a.wts[(size_t)t0 * F + e] : 1.0f;
    fill(sd, dz + (size_t)t0 * a.D0p, 16 * a.D0p / 4);
    __syncthreads();
    for (int c = tid; c < FS; c += 256) {                        // a thread owns (field f, slot l) for all 16 examples:
        const int f = c / SLOT, l = c % SLOT;                    // the pair index is computed once per partner field
        float g[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = l < K ? sd[r * a.D0p + c] : 0.f;
        if (l < K && P) {
            for (int j = 0; j < F; ++j) {
                // pair (i, j), i < j, sits at FS + i*(2F - i - 1)/2 + (j - i - 1); j == f contributes nothing
                const int i0 = f < j ? f : j, j0 = f < j ? j : f;
                const int n = j == f ? 0 : i0 * (2 * F - i0 - 1) / 2 + (j0 - i0 - 1);
                const float on = j == f ? 0.f : 1.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) g[r] = fmaf(sd[r * a.D0p + FS + n] * on, se[r * FS + j * SLOT + l], g[r]);
            }
        }
        if (WV) {
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] *= sw[r * F + f];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) gxp[(size_t)(t0 + r) * a.D0p + c] = g[r];
    }
    if (tid == 0) { float s = 0.f; for (int r = 0; r < 16; ++r) s += sd[r * a.D0p + CB]; gb_part[blockIdx.x] = s; }
