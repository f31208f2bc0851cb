// ip_update_all_code.inc.h -- the code of k_ip_update_all<T> (ip_step_kernels.hip.h), included inside the solo kernel and inside its group
// form k_ip_update_all_g (ip_group_kernels.hip.h): `u` (IpUpdArgs) and T are the including function's; the last workgroup of x leaves through UPDATE_ALL_DONE.
// Text, not a __device__ function, for the reason ip_bwd_code.inc.h gives.
    if (blockIdx.x == gridDim.x - 1) {               // scalar tail: the loss, a fixed-shape tree (b: k_ip_b_update)
        __shared__ float sl[256];
        sl[threadIdx.x] = strided_sum256(u.loss_t, u.Ba); __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) sl[threadIdx.x] += sl[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) { *u.loss_sum = sl[0]; UPDATE_ALL_DONE(sl[0]); }
        return;
    }
    // A workgroup owns a 64 x 64 tile of one layer's W (row lengths are multiples of 64); a thread 4 consecutive elements
    // of 4 rows: 16-byte slab / master / state accesses and 8-byte pieces of the backward shadow (k = column).  The forward
    // shadow has k = row: the tile goes through LDS transposed and leaves as whole 16-byte lane slots.
    typedef typename Traits<T>::frag frag;
    constexpr int EPL = Traits<T>::EPL;
    __shared__ __align__(16) T sT[64][64 + EPL];                 // [column][row], padded
    const size_t tile = blockIdx.x;
    if (tile * 4096 >= u.off[u.n]) return;
    if (*u.err & 2) return;                                      // a strip pair gave up (StripDuo): the gradients are garbage, the weights stay
    int t = 0;
#pragma unroll
    for (int q = 1; q <= IPNN_MAX_HIDDEN; ++q) t += (q < u.n && tile * 4096 >= u.off[q]) ? 1 : 0;
    const int Dout = u.Dout[t], Din = u.Din[t], ntc = Dout / 64;
    const int lt = (int)(tile - u.off[t] / 4096), r0 = (lt / ntc) * 64, c0 = (lt % ntc) * 64;
    const int cq = (threadIdx.x & 15) * 4, sk = u.sk[t];
    T* wb = static_cast<T*>(u.wb[t]);
    // the split-K slabs of the thread's 4 x 4 elements, summed in slab order: the loads of four slabs x four rows are issued
    // together (a `for z: load, add` loop pays one memory round trip per slab and row: 21 -> 17 us for the whole launch)
    float4 gs[4], ws[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        gs[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        ws[k] = *reinterpret_cast<const float4*>(u.W[t] + (size_t)(r0 + (threadIdx.x >> 4) + 16 * k) * Dout + c0 + cq);
    }
    for (int z0 = 0; z0 < sk; z0 += 4) {
        float4 v[4][4];
#pragma unroll
        for (int zz = 0; zz < 4; ++zz)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const size_t i = u.off[t] + (size_t)(r0 + (threadIdx.x >> 4) + 16 * k) * Dout + c0 + cq;
                v[zz][k] = z0 + zz < sk ? *reinterpret_cast<const float4*>(u.slab + (size_t)(z0 + zz) * u.zstride + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
        for (int zz = 0; zz < 4; ++zz)
#pragma unroll
            for (int k = 0; k < 4; ++k) { gs[k].x += v[zz][k].x; gs[k].y += v[zz][k].y; gs[k].z += v[zz][k].z; gs[k].w += v[zz][k].w; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + (threadIdx.x >> 4) + 16 * k, c = c0 + cq;
        const size_t j = (size_t)r * Dout + c;
        const float4 g = gs[k];
        float4 w = ws[k];
        if (u.adam) {
            float4 m = *reinterpret_cast<const float4*>(u.Wm[t] + j), v = *reinterpret_cast<const float4*>(u.Wv[t] + j);
            w.x = opt_step(u.adam, w.x, g.x, m.x, v.x, u.lr, u.beta1, u.beta2, u.eps);
            w.y = opt_step(u.adam, w.y, g.y, m.y, v.y, u.lr, u.beta1, u.beta2, u.eps);
            w.z = opt_step(u.adam, w.z, g.z, m.z, v.z, u.lr, u.beta1, u.beta2, u.eps);
            w.w = opt_step(u.adam, w.w, g.w, m.w, v.w, u.lr, u.beta1, u.beta2, u.eps);
            *reinterpret_cast<float4*>(u.Wm[t] + j) = m; *reinterpret_cast<float4*>(u.Wv[t] + j) = v;
        } else { w.x -= u.lr * g.x; w.y -= u.lr * g.y; w.z -= u.lr * g.z; w.w -= u.lr * g.w; }
        store16_sel(u.wt, u.W[t] + j, w);                       // (written through: see store4_wt)
        store4_sel(u.wt, wb + ft_off<T>(r, c, Dout), w.x, w.y, w.z, w.w);
        const int rl = r - r0;
        sT[cq][rl] = (T)w.x; sT[cq + 1][rl] = (T)w.y; sT[cq + 2][rl] = (T)w.z; sT[cq + 3][rl] = (T)w.w;
    }
    __syncthreads();
    T* wf = static_cast<T*>(u.wf[t]);
    for (int e = threadIdx.x; e < 64 * (64 / EPL); e += 256) {      // (column, group of EPL rows): one lane slot of wf
        const int cl = e & 63, g8 = e >> 6;
        store16_sel(u.wt, wf + ft_off<T>(c0 + cl, r0 + g8 * EPL, Din), *reinterpret_cast<const frag*>(&sT[cl][g8 * EPL]));
    }
