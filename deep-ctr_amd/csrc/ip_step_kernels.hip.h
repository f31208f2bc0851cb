// ip_step_kernels.hip.h -- what a training step of the inner-product family runs around the gather and the stack (gfx950
// only).  A part of the unit ipnn_api.hip, which alone includes it.
//   k_mask_T, k_mask_draw        the keep-masks of a step, transposed from the caller's or drawn on the device (ip_masks,
//                                ipnn_draw_masks)
//   k_ip_update, k_fill_f32      a weight's tiled shadows refreshed (ip_refresh); a constant fill (ipnn_set_table)
//   k_adam_table, k_ip_b_update  the table pass and the scalar b of an Adam / FTRL or SGD step (ip_adam_table, ip_b_update)
//   k_ip_update_all              the dense update of the whole stack and the loss sum in one launch (ip_dense_update); its
//                                code is ip_update_all_code.inc.h, shared as text with the group form k_ip_update_all_g
// The launchers named are ipnn_api.hip's; the *_body functions are also the bodies of the group forms (ip_group_kernels.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ipnn_hip.h"
#include "fnn_kernels.hip.h"
#include "ip_gather_kernels.hip.h"     // ipw_u32x4
#include "ip_strip_kernels.hip.h"      // mask_off: the layout of the transposed masks that the epilogues read
#include "optim.hip.h"

namespace {
using namespace fnn;

// Keep-masks [B][d] uint8 (the ABI's layout, reference column order) -> [Dp][ldT] uint8, zero padded,
// for every layer in one launch; layer 0's columns are mapped to the slot layout on the way.
struct MaskTArgs {
    const uint8_t* src[IPNN_MAX_HIDDEN + 1]; uint8_t* dst[IPNN_MAX_HIDDEN + 1]; int d[IPNN_MAX_HIDDEN + 1], Dp[IPNN_MAX_HIDDEN + 1];
    int tile0[IPNN_MAX_HIDDEN + 2]; int n; const int* ref0; int B, Ba, ldT; bool wt;
};
// (the body of k_mask_T and of its group form k_mask_T_g.  A: how the arguments arrive -- `const MaskTArgs`, the kernel's own
// parameter, in the solo kernel; `const MaskTArgs&`, the member's record in memory, in the group form.  mask_draw_body likewise.)
template <typename A> __device__ __forceinline__ void mask_T_body(A a)
{
    __shared__ __align__(4) uint8_t s[64][68];          // 17 dwords per row: the 64 lanes of a byte store (one row each) spread over all banks
    int t = 0;
#pragma unroll
    for (int q = 1; q <= IPNN_MAX_HIDDEN; ++q) t += (q < a.n && (int)blockIdx.x >= a.tile0[q]) ? 1 : 0;
    const int local = (int)blockIdx.x - a.tile0[t], ntx = a.Ba / 64;
    const int t0 = (local % ntx) * 64, c0 = (local / ntx) * 64;
    {   // a thread's column is the same in all 16 of its elements (i = tid + 256 k): its source column once, then all
        // 16 bytes in one round trip, then the LDS transposition
        // (four such tiles per workgroup, 64 loads in flight per thread, changed nothing: 12.0 against 12.2 us -- not a latency chain)
        const int cx = threadIdx.x & 63, c = c0 + cx, d = a.d[t];
        int sc = c < a.Dp[t] ? c : -1;
        if (t == 0) sc = sc >= 0 ? a.ref0[sc] : -1; else if (sc >= d) sc = -1;
        const uint8_t* __restrict__ src = a.src[t] + (sc >= 0 ? sc : 0);
        uint8_t v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int ex = t0 + (threadIdx.x >> 6) + 4 * k;
            v[k] = (ex < a.B && sc >= 0) ? src[(size_t)ex * d] : (uint8_t)0;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) s[cx][(threadIdx.x >> 6) + 4 * k] = v[k];
    }
    __syncthreads();
    const int cc = threadIdx.x >> 2, q = threadIdx.x & 3;
    if (c0 + cc < a.Dp[t])
    {
        const unsigned* w = reinterpret_cast<const unsigned*>(&s[cc][16 * q]);
        store16_sel(a.wt, a.dst[t] + mask_off(c0 + cc, t0 + 16 * q, a.ldT), make_uint4(w[0], w[1], w[2], w[3]));
    }
}
static __global__ __launch_bounds__(256) void k_mask_T(const MaskTArgs a) { mask_T_body<const MaskTArgs>(a); }

// Drawn keep-masks (ipnn_train_step_drawn / ipnn_draw_masks): the generator that stands where k_mask_T stands.  The mask of
// (layer t, example ex, reference column c) is one 32-bit word of Philox4x32-10 (Salmon et al., SC'11) against a threshold:
//   key = (lo32(seed), hi32(seed)), counter = (c, t << 16 | ex >> 2, lo32(step), hi32(step)), word j <-> example 4 (ex >> 2) + j
// (include/ipnn_hip.h; deep-ctr_amd/dropout.py restates it in NumPy and the tests hold the two equal byte for byte).
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned w[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}
// One launch for every layer, tiled like k_mask_T (64 columns x 64 examples a workgroup).  A thread owns one column and 16
// consecutive examples: four Philox calls, one 16-byte slot of the transposed layout dstT[t] ([Dp][ldT], mask_off; pad columns
// and the examples from B on are zero, layer 0 in slot order with the draw taken at the slot's reference column) -- written
// exactly as k_mask_T writes it, but with nothing read.  dstR[t], where set, takes the same bytes row-major in the ABI's layout
// ([B][d_t], reference column order) through an LDS transposition: layer 0 of a training step (the inner-product forward reads
// it through its `mask` argument), every layer for ipnn_draw_masks.  The stores are plain C++ or raw buffer stores with the sc1
// policy (see ipw_store16), never inline assembly.
struct MaskDrawArgs {
    uint8_t* dstT[IPNN_MAX_HIDDEN + 1]; uint8_t* dstR[IPNN_MAX_HIDDEN + 1]; int d[IPNN_MAX_HIDDEN + 1], Dp[IPNN_MAX_HIDDEN + 1];
    unsigned bytesT[IPNN_MAX_HIDDEN + 1];       // extent of dstT[t]: the write-through stores' buffer resource
    int tile0[IPNN_MAX_HIDDEN + 2]; int n; const int* ref0; int B, Ba, ldT; bool wt;
    unsigned key0, key1, step0, step1, thr; bool all;      // all: keep_prob >= 1, every element is kept
};
// (the body of k_mask_draw and of its group form k_mask_draw_g)
template <typename A> __device__ __forceinline__ void mask_draw_body(A a)
{
    __shared__ __align__(16) uint8_t s[64][68];         // [column][example], 17 dwords per row (k_mask_T's tile)
    int t = 0;
#pragma unroll
    for (int q = 1; q <= IPNN_MAX_HIDDEN; ++q) t += (q < a.n && (int)blockIdx.x >= a.tile0[q]) ? 1 : 0;
    uint8_t* const dT = a.dstT[t];
    uint8_t* const dR = a.dstR[t];
    if (!dT && !dR) return;
    const int local = (int)blockIdx.x - a.tile0[t], ntx = a.Ba / 64;
    const int t0 = (local % ntx) * 64, c0 = (local / ntx) * 64, d = a.d[t];
    {
        const int cc = threadIdx.x >> 2, q = threadIdx.x & 3, c = c0 + cc, ex0 = t0 + 16 * q;
        int sc = t == 0 ? a.ref0[c] : (c < d ? c : -1);             // c < Dp[t]: the tiles cover exactly the padded columns
        ipw_u32x4 v = {0u, 0u, 0u, 0u};
        if (sc >= 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ex = ex0 + 4 * j;
                if (ex >= a.B) continue;
                unsigned w[4] = {0u, 0u, 0u, 0u};
                if (!a.all) philox4x32_10((unsigned)sc, ((unsigned)t << 16) | (unsigned)(ex >> 2), a.step0, a.step1, a.key0, a.key1, w);
                unsigned pk = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) pk |= ((ex + i < a.B && (a.all || w[i] < a.thr)) ? 1u : 0u) << (8 * i);
                v[j] = pk;
            }
        }
        if (dT) ipw_store16(a.wt, ipw_rsrc(dT, a.bytesT[t]), dT, mask_off(c, ex0, a.ldT), v);
        if (dR) {                                                    // 68 cc + 16 q is a multiple of 4 only: four dword stores
            unsigned* sw = reinterpret_cast<unsigned*>(&s[cc][16 * q]);
#pragma unroll
            for (int j = 0; j < 4; ++j) sw[j] = v[j];
        }
    }
    if (!dR) return;
    __syncthreads();
    const int cx = threadIdx.x & 63, c = c0 + cx;
    const int sc = t == 0 ? a.ref0[c] : (c < d ? c : -1);
    if (sc < 0) return;
#pragma unroll
    for (int k = 0; k < 16; ++k) {                                   // a wave writes 64 columns of one example: one run per field
        const int r = (threadIdx.x >> 6) + 4 * k, ex = t0 + r;
        if (ex < a.B) dR[(size_t)ex * d + sc] = s[cx][r];
    }
}
static __global__ __launch_bounds__(256) void k_mask_draw(const MaskDrawArgs a) { mask_draw_body<const MaskDrawArgs>(a); }

// W_t <- W_t - lr * sum of slabs; refresh both tiled shadows.  Layer 1 rows are in slot layout.
template <typename T>
static __global__ void k_ip_update(float* __restrict__ W, const float* __restrict__ slab, int splitk, size_t zstride,
                                   float lr, int Din, int Dout, T* __restrict__ wf, T* __restrict__ wb)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)Din * Dout) return;
    float w = W[i];
    if (slab) {
        float g = 0.f;
        for (int z = 0; z < splitk; ++z) g += slab[(size_t)z * zstride + i];
        w -= lr * g; W[i] = w;
    }
    const int r = (int)(i / Dout), c = (int)(i % Dout);
    wf[ft_off<T>(c, r, Din)] = (T)w;
    wb[ft_off<T>(r, c, Dout)] = (T)w;
}
__device__ inline float opt_step(int opt, float w, float g, float& s0, float& s1, float lr, float b1, float b2, float eps) {
    return opt == IPNN_OPT_FTRL ? ftrl_step(w, g, s0, s1, lr) : adam_step(w, g, s0, s1, lr, b1, b2, eps);
}

static __global__ void k_fill_f32(float* __restrict__ p, size_t n, float v)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// Adam on the embedding table: TensorFlow's gradient through concat / slice is DENSE (zero for
// untouched rows), so every row's moments decay and every row moves each step -- one streaming pass
// over table, m, v and the per-row gradient sums G (which it zeroes again for the next step).
// (FTRL: the same pass with (accum, linear) in place of the moments.)
static __global__ void k_adam_table(float* __restrict__ tab, float* __restrict__ m, float* __restrict__ v, float* __restrict__ G,
                                    size_t n, float lr_t, float b1, float b2, float eps, int opt)
{
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    float4 w = *reinterpret_cast<float4*>(tab + i), mm = *reinterpret_cast<float4*>(m + i), vv = *reinterpret_cast<float4*>(v + i);
    const float4 g = *reinterpret_cast<const float4*>(G + i);
    w.x = opt_step(opt, w.x, g.x, mm.x, vv.x, lr_t, b1, b2, eps); w.y = opt_step(opt, w.y, g.y, mm.y, vv.y, lr_t, b1, b2, eps);
    w.z = opt_step(opt, w.z, g.z, mm.z, vv.z, lr_t, b1, b2, eps); w.w = opt_step(opt, w.w, g.w, mm.w, vv.w, lr_t, b1, b2, eps);
    *reinterpret_cast<float4*>(tab + i) = w; *reinterpret_cast<float4*>(m + i) = mm; *reinterpret_cast<float4*>(v + i) = vv;
    *reinterpret_cast<float4*>(G + i) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// One launch for the whole stack: W_t <- W_t - lr * (sum of its split-K slabs), both tiled shadows
// refreshed; the last workgroup applies the bias-of-z1 gradient and reduces the per-example losses.
struct IpUpdArgs {
    bool wt;                                         // weights and shadows written through (IPNN_WT)
    float* W[IPNN_MAX_HIDDEN + 1]; void* wf[IPNN_MAX_HIDDEN + 1]; void* wb[IPNN_MAX_HIDDEN + 1];
    size_t off[IPNN_MAX_HIDDEN + 2];                 // element offset of every layer in a slab; off[n] = total
    int Din[IPNN_MAX_HIDDEN + 1], Dout[IPNN_MAX_HIDDEN + 1], sk[IPNN_MAX_HIDDEN + 1]; int n;
    const float* slab; size_t zstride; float lr;
    float* b; const float* gb_part; int ngb; const float* loss_t; int Ba; float* loss_sum;
    // Adam (python/tf_util.py:17-20, TensorFlow's AdamOptimizer): first / second moments beside every tensor;
    // lr is then lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) of this step
    int adam;                                        // 0 = SGD, else IPNN_OPT_ADAM / IPNN_OPT_FTRL (state = (accum, linear))
    float beta1, beta2, eps; float* Wm[IPNN_MAX_HIDDEN + 1]; float* Wv[IPNN_MAX_HIDDEN + 1]; float* bmv;
    const int* err;                                  // bit 1 set (a strip pair gave up its swap): the step's activations are invalid -- nothing is applied
};

// The scalar b of z1 (python/FNN_IP_L7.py:104-114): its gradient is the sum of the per-workgroup partials of k_ip_bwd.  A launch
// of its own on the side stream, right behind k_ip_bwd, so that the dense update on the main stream depends on nothing there.
struct IpBArgs { float* b; const float* gb_part; int ngb, opt; float* bmv; float lr, beta1, beta2, eps; const int* err; };
// (the body of k_ip_b_update and of its group form k_ip_b_update_g)
__device__ __forceinline__ void ip_b_update_body(float* __restrict__ b, const float* __restrict__ gb_part, int ngb, int opt,
                                                 float* __restrict__ bmv, float lr, float beta1, float beta2, float eps, const int* __restrict__ err)
{
    __shared__ float sg[256];
    if (*err & 2) return;
    sg[threadIdx.x] = strided_sum256(gb_part, ngb);
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sg[threadIdx.x] += sg[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (opt) *b = opt_step(opt, *b, sg[0], bmv[0], bmv[1], lr, beta1, beta2, eps);
        else *b -= lr * sg[0];
    }
}
static __global__ __launch_bounds__(256) void k_ip_b_update(float* __restrict__ b, const float* __restrict__ gb_part, int ngb, int opt,
                                                            float* __restrict__ bmv, float lr, float beta1, float beta2, float eps, const int* __restrict__ err)
{
    ip_b_update_body(b, gb_part, ngb, opt, bmv, lr, beta1, beta2, eps, err);
}

#define UPDATE_ALL_DONE(loss) do { } while (0)
template <typename T>
static __global__ __launch_bounds__(256) void k_ip_update_all(const IpUpdArgs u)
{
#include "ip_update_all_code.inc.h"
}
#undef UPDATE_ALL_DONE

}  // namespace
