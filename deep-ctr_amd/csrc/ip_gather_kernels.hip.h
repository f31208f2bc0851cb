// ip_gather_kernels.hip.h -- the inner-product layer of the FNN_IP family (gfx950 only): the gather of a batch's rows, the
// pair products and the first activation, forward and backward, in the three forms the row width and the field count choose
// between.  A part of the unit ipnn_api.hip, which alone includes it (the unit's flags keep the MFMA accumulators in VGPRs).
//   k_ip_fwd / k_ip_bwd          narrow rows (k <= 16): 16 examples per workgroup, a0 staged in LDS.  The backward's code is
//                                ip_bwd_code.inc.h, shared as text with the group form k_ip_bwd_g.
//   k_ip_fwd_w / k_ip_bwd_w      wide rows (k = 17 .. 128): IPW_EX examples per workgroup, a0 computed in registers; with
//                                k_ip_scatw1 / k_ip_scatw2, the sparse-row update on rows of that width.
//   k_ip_fwd_m / k_ip_bwd_m      narrow rows of 33 .. 64 fields, where the 16-example tile is too large or measured slower
//                                (ip_many_choice): IPM_EX / IPM_BEX examples per workgroup.
// In front of them the activation helpers (ip_act ...) that the strip kernels' epilogues use too.  The host side picks a form
// in ip_fwd_rows / ip_bwd_rows and launches it from ip_gather_fwd and ip_side_chain (ipnn_api.hip, through the selectors
// ip_gather_fwd_sel ...); the *_body functions are also the bodies of the group forms (ip_group_kernels.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ipnn_hip.h"
#include "fnn_kernels.hip.h"
#include "sparse_rows.hip.h"

namespace {
using namespace fnn;

constexpr int A_TANH = IPNN_ACT_TANH, A_SIG = IPNN_ACT_SIGMOID, A_RELU = IPNN_ACT_RELU;

__device__ inline float ip_act(float z, int act) {
    if (act == A_RELU) return fmaxf(z, 0.f);
    if (act == A_TANH) return tanhf(z);
    return 1.0f / (1.0f + expf(-z));
}
template <int ACT> __device__ inline float ip_act_c(float z) {
    if (ACT == A_RELU) return fmaxf(z, 0.f);
    if (ACT == A_TANH) return tanhf(z);
    return 1.0f / (1.0f + expf(-z));
}
template <int ACT> __device__ inline float ip_dact_u_c(float u) {
    if (ACT == A_RELU) return u > 0.f ? 1.0f : 0.0f;
    if (ACT == A_TANH) return 1.0f - u * u;
    return u * (1.0f - u);
}
// derivative of act at l, written in terms of u = act(l)
__device__ inline float ip_dact_u(float u, int act) {
    if (act == A_RELU) return u > 0.f ? 1.0f : 0.0f;
    if (act == A_TANH) return 1.0f - u * u;
    return u * (1.0f - u);
}

// ------------------------------------------------------------------------------------------
// Inner-product layer, forward (python/FNN_IP_L7.py:104-114 + the first act/dropout of :115):
// 16 examples per workgroup.  a0' [Ba][D0p] in "slot" layout: column 16 f + l = e_f[l],
// columns 16F .. 16F+P-1 the P = F(F-1)/2 pair products (row-major i < j), column CB = b,
// column CB+1 = 1 (carries h1_b); every real column goes through act and the keep-mask / keep.
// a0 is written fragment-tiled twice: a0F (rows = examples, k = columns: the next forward product's
// A operand) and a0T (rows = columns, k = examples: the weight-gradient product's A operand).
// ------------------------------------------------------------------------------------------
struct IpFwdArgs {
    int P;                      // pair products: F (F - 1) / 2 (FNN_IP_L*) or 0 (the plain FNN class, python/FNN.py:80)
    const int32_t* ids; int B, F, K; const float* table16; int64_t n_rows; const float* b;
    const uint8_t* mask; int d0; float inv_keep; int act; int D0p, ldT; int* err;
    int skip;                   // diagnostics (IPNN_FWD_SKIP bits: 1 gather, 2 embedding store, 4 compute, 8 output stores); 0 in production
    bool wt;                    // outputs written through (IPNN_WT=0: plain stores; see store4_wt in fnn_kernels.hip.h)
    const float* wts;           // value weights [B][F] (read by the WV variant only; NULL: every weight 1)
};

// gather of 16 examples' rows into an LDS tile [16][F*16]: all ids of a batch of 4 elements per thread first, then all
// rows (two dependent round trips per batch instead of two per element)
// STR: floats per field in the tile -- 16 (vector stores), or 17 for the forward's pair products: lanes that read slot l of
// DIFFERENT fields then fall on different banks (with 16 all of them share two banks: a 32-way conflict per read)
// WV: value weights (ipnn_*_w with wts != NULL): the weight of (example t, field f) sits at the id's own index, is loaded in the id's
// round trip and scales the row's pieces in f32, so that the tile -- and emb, copied from it -- holds e_f = wts[t][f] * row
template <int STR, int NT = 256, bool WV = false>
__device__ __forceinline__ void ip_gather16(float* se, const int32_t* __restrict__ ids, const float* __restrict__ table16,
                                            const int64_t n_rows, const int t0, const int B, const int F, int* err,
                                            const float* __restrict__ wts = nullptr)
{
    const int n = 16 * F * 4, FS = F * STR;
    for (int e0 = threadIdx.x; e0 < n; e0 += NT * 4) {
        int64_t id[4];
        float w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + NT * j, f = (e >> 2) % F, t = t0 + (e >> 2) / F;
            id[j] = (e < n && t < B) ? (int64_t)ids[(size_t)t * F + f] : -1;
            if (WV) w[j] = (e < n && t < B) ? wts[(size_t)t * F + f] : 0.f;
        }
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + NT * j;
            if (e < n && t0 + (e >> 2) / F < B && (id[j] < 0 || id[j] >= n_rows)) { if (err) atomicOr(err, 1); id[j] = -1; }
            v[j] = id[j] >= 0 ? *reinterpret_cast<const float4*>(table16 + (size_t)id[j] * SLOT + 4 * (e & 3)) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (WV && id[j] >= 0) { v[j].x *= w[j]; v[j].y *= w[j]; v[j].z *= w[j]; v[j].w *= w[j]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + NT * j;
            if (e < n) {
                float* d = se + ((e >> 2) / F) * FS + ((e >> 2) % F) * STR + 4 * (e & 3);
                if (STR == SLOT) *reinterpret_cast<float4*>(d) = v[j];
                else { d[0] = v[j].x; d[1] = v[j].y; d[2] = v[j].z; d[3] = v[j].w; }
            }
        }
    }
}

constexpr int IPF_NT = 512;     // 8 waves: the kernel is bound by instruction issue, two waves per SIMD overlap it (IPNN_IPF_NT=1024: four)
// (the body of k_ip_fwd and of its group form k_ip_fwd_g; TL = false: the T layout a0T is not written -- a prediction reads a0 only)
template <typename T, int NT, bool WV, bool TL = true>
__device__ __forceinline__ void ip_fwd_body(const IpFwdArgs& a, T* __restrict__ a0, T* __restrict__ a0T, float* __restrict__ emb)
{
    typedef typename Traits<T>::frag frag;
    constexpr int EPL = Traits<T>::EPL;
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int SP = SLOT + 1;                                // padded field stride of the embedding tile
    float* se = reinterpret_cast<float*>(smem);                 // [16][F*17] raw embeddings
    float* sa = se + 16 * a.F * SP;                             // [16][D0p]  a0 values
    const int tid = threadIdx.x, t0 = blockIdx.x * 16, F = a.F, K = a.K, B = a.B, FS = F * SLOT, FSP = F * SP;
    const int P = a.P, CB = FS + P;
    if (!(a.skip & 1)) ip_gather16<SP, NT, WV>(se, a.ids, a.table16, a.n_rows, t0, B, F, a.err, a.wts);
    __syncthreads();
    if (emb && !(a.skip & 2))                                                    // kept for the backward of the inner products (no second gather; WV: weighted)
        for (int e = tid; e < 16 * FS / 4; e += NT) {
            const int r = (4 * e) / FS, c = (4 * e) % FS;
            const float* q = se + r * FSP + (c >> 4) * SP + (c & 15);
            store16_sel(a.wt, emb + (size_t)t0 * FS + 4 * e, make_float4(q[0], q[1], q[2], q[3]));
        }
    const float bval = *a.b;
    // a thread owns columns c = (tid & 63) + 64 k and rows r = (tid >> 6) + NWV i; 8 columns at a time: their pair indices,
    // then all 8 RPT keep-mask bytes (one round trip), then the values
    constexpr int NWV = NT / 64, RPT = 16 / NWV;
    for (int c0 = tid & 63; c0 < ((a.skip & 4) ? 0 : a.D0p); c0 += 512) {
        int ref[8], pi[8], pj[8];                               // ref: column in the reference's z1 order
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = c0 + 64 * k;
            ref[k] = -1; pi[k] = 0; pj[k] = 0;
            if (c < FS) { const int f = c / SLOT, l = c % SLOT; if (l < K) ref[k] = f * K + l; }
            else if (c < CB) {
                int n = c - FS, i = 0;                          // n-th pair (i, j), i < j, row-major
                while (n >= F - 1 - i) { n -= F - 1 - i; ++i; }
                pi[k] = i; pj[k] = i + 1 + n; ref[k] = F * K + (c - FS);
            } else if (c == CB) ref[k] = a.d0 - 1;
        }
        float mk[8][RPT];
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                const int t = t0 + (tid >> 6) + NWV * i;
                mk[k][i] = (a.mask && ref[k] >= 0 && t < B) ? (float)a.mask[(size_t)t * a.d0 + ref[k]] * a.inv_keep : 1.0f;
            }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = c0 + 64 * k;
            if (c >= a.D0p) break;
#pragma unroll
            for (int i = 0; i < RPT; ++i) {
                const int r = (tid >> 6) + NWV * i, t = t0 + r;
                float z = 0.f;
                if (c < FS) z = se[r * FSP + (c >> 4) * SP + (c & 15)];
                else if (c < CB) {
                    float s2 = 0.f;
                    for (int l = 0; l < K; ++l) s2 = fmaf(se[r * FSP + pi[k] * SP + l], se[r * FSP + pj[k] * SP + l], s2);
                    z = s2;
                } else if (c == CB) z = bval;
                float v = 0.f;
                if (t < B) {
                    if (ref[k] >= 0) v = ip_act(z, a.act) * mk[k][i];
                    else if (c == CB + 1) v = 1.0f;
                }
                sa[r * a.D0p + c] = v;
            }
        }
    }
    __syncthreads();
    // F layout: this workgroup's 16 rows are one row tile; a lane-slot of a fragment = EPL consecutive columns of one row
    if (a.skip & 8) return;
    for (int e = tid; e < 16 * a.D0p / EPL; e += NT) {
        const int g = e >> 4, r = e & 15;                        // column group, row
        frag fv;
#pragma unroll
        for (int x = 0; x < EPL; ++x) fv[x] = (T)sa[r * a.D0p + g * EPL + x];
        store16_sel(a.wt, a0 + ft_off<T>(t0 + r, g * EPL, a.D0p), fv);
    }
    if (!TL) return;
    for (int e = tid; e < a.D0p * 4; e += NT) {
        const int c = e >> 2, tq = e & 3;
        store4_sel(a.wt, a0T + ft_off<T>(c, t0 + 4 * tq, a.ldT), sa[(4 * tq) * a.D0p + c], sa[(4 * tq + 1) * a.D0p + c],
                  sa[(4 * tq + 2) * a.D0p + c], sa[(4 * tq + 3) * a.D0p + c]);
    }
}
template <typename T, int NT = IPF_NT, bool WV = false>
static __global__ __launch_bounds__(NT) void k_ip_fwd(const IpFwdArgs a, T* __restrict__ a0, T* __restrict__ a0T, float* __restrict__ emb)
{
    ip_fwd_body<T, NT, WV>(a, a0, a0T, emb);
}

// Inner-product layer, backward: dz1' [Ba][D0p] f32 (already times mask/keep and act') ->
// slot-layout embedding gradients gx' [Ba][D0p] (columns 16f + l) for the sparse-row update, and the
// per-workgroup partial of db = sum_t dz1[b].
// WV (value weights): emb holds the weighted embeddings, so the partner reads are unchanged; the finished gradient of (field f,
// example t) is the gradient of e_f, and its row's is that times wts[t][f].  The 16 x F weights of the tile are staged in the F
// floats per example that the launch's LDS size (k_ip_fwd's: a 17-float field stride) leaves behind sd.
struct IpBwdArgs { int P; const int32_t* ids; int B, F, K; const float* table16; int64_t n_rows; int D0p; const float* emb; const float* wts; };

template <bool WV = false>
static __global__ __launch_bounds__(256) void k_ip_bwd(const IpBwdArgs a, const float* __restrict__ dz, float* __restrict__ gxp,
                                                        float* __restrict__ gb_part)
{
#include "ip_bwd_code.inc.h"
}

// ------------------------------------------------------------------------------------------
// Wide rows (k = 17 .. 128, FM50 / FM100 seeds): the same layer on rows of rw = rup(k, 4) floats.  Layer 0 column f rw + l
// holds e_f[l], then the P pair products, b and the ones column: D0p = rup(F rw + P + 2, 64).  k_ip_fwd's tile (16 examples x
// (17 F + D0p) floats) does not fit the LDS there -- 220 KB at F = 16, k = 101, ~560 KB at F rw = 4096 -- so a workgroup takes
// IPW_EX = 8 examples and stages only their embeddings (F (rw + 1) floats each, <= 132 KB).  Each a0 value is computed in
// registers: a thread owns EPL consecutive columns of the 8 examples, which is one lane slot of every example's F-layout row and
// whole lane slots of the T layout (bf16: 8 examples = one 16-byte slot, so no slot is shared by two workgroups), so a0 needs no
// LDS tile at all.
// ------------------------------------------------------------------------------------------
constexpr int IPW_EX = 8;       // examples per workgroup of the wide inner-product launches
struct IpWideArgs {
    int P; const int32_t* ids; int B, F, K, rw; const float* table; int64_t n_rows; const float* b;
    const uint8_t* mask; int d0; float inv_keep; int act; int D0p, ldT; int* err;
    bool wt;                    // outputs written through (IPNN_WT=0: plain stores)
    unsigned a0_bytes, emb_bytes;   // sizes of a0 / a0T and of emb: the extent of the write-through stores' buffer resources
    const float* wts;           // value weights [B][F] (read by the WV variants only; NULL: every weight 1)
};
// The wide kernels' write-through stores are raw buffer stores with the sc1 policy (aux 16), not the inline-asm store16_wt /
// store4_wt: hipcc neither counts nor pads an asm store, so the instruction after a `global_store_dwordx4` there may overwrite its
// data registers before the store has read them -- in k_ip_fwd_w<bf16_t> that happened (a0 differed between identical runs).
typedef unsigned int ipw_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int ipw_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ipw_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
template <typename V> __device__ __forceinline__ void ipw_store16(const bool wt, const __amdgpu_buffer_rsrc_t rs, void* base, const size_t off, const V& v) {
    static_assert(sizeof(V) == 16, "ipw_store16: 16-byte values");
    ipw_u32x4 w; __builtin_memcpy(&w, &v, 16);
    if (wt) __builtin_amdgcn_raw_buffer_store_b128(w, rs, (int)off, 0, 16);
    else *reinterpret_cast<ipw_u32x4*>(static_cast<char*>(base) + off) = w;
}
// four consecutive k of a fragment-tiled operand: 16 bytes (f32) or 8 (bf16)
__device__ __forceinline__ void ipw_store4(const bool wt, const __amdgpu_buffer_rsrc_t rs, float* base, const size_t e, float a, float b, float c, float d) {
    ipw_store16(wt, rs, base, e * 4, make_float4(a, b, c, d));
}
__device__ __forceinline__ void ipw_store4(const bool wt, const __amdgpu_buffer_rsrc_t rs, bf16_t* base, const size_t e, float a, float b, float c, float d) {
    bf16x4 v = {(bf16_t)a, (bf16_t)b, (bf16_t)c, (bf16_t)d};
    ipw_u32x2 w; __builtin_memcpy(&w, &v, 8);
    if (wt) __builtin_amdgcn_raw_buffer_store_b64(w, rs, (int)(e * 2), 0, 16);
    else *reinterpret_cast<ipw_u32x2*>(base + e) = w;
}
inline size_t ipw_fwd_lds(int F, int rw) { return (size_t)IPW_EX * F * (rw + 1) * sizeof(float); }
inline size_t ipw_bwd_lds(int F, int rw, int P, bool wv) { return (size_t)IPW_EX * (F * rw + P + (wv ? F : 0)) * sizeof(float); }

// WV (value weights, here and in k_ip_bwd_w / k_ip_fwd_m / k_ip_bwd_m): as in ip_gather16 and k_ip_bwd -- every 16-byte piece of a
// gathered row is scaled by wts[t][f] before it goes to the tile and to emb; the backward scales its finished gradient once.
template <typename T, bool WV, bool TL = true>
__device__ __forceinline__ void ip_fwd_w_body(const IpWideArgs& a, T* __restrict__ a0, T* __restrict__ a0T, float* __restrict__ emb)
{
    typedef typename Traits<T>::frag frag;
    constexpr int EPL = Traits<T>::EPL;
    extern __shared__ __align__(16) unsigned char smem[];
    float* se = reinterpret_cast<float*>(smem);                 // [IPW_EX][F][rw + 1]: the odd stride spreads the pair reads of a wave
    const int F = a.F, K = a.K, rw = a.rw, SW = rw + 1, nq = rw >> 2, FW = F * rw, CB = FW + a.P, B = a.B;
    const int t0 = blockIdx.x * IPW_EX;
    const __amdgpu_buffer_rsrc_t r_emb = ipw_rsrc(emb, a.emb_bytes), r_a0 = ipw_rsrc(a0, a.a0_bytes), r_a0T = ipw_rsrc(a0T, a.a0_bytes);
    // gather: IPW_EX x F rows of nq 16-byte pieces, four in flight per thread; the raw rows also go to emb (the backward's copy)
    const int n = IPW_EX * F * nq;
    for (int e0 = threadIdx.x; e0 < n; e0 += 256 * 4) {
        int64_t id[4];
        float w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + 256 * j, t = t0 + e / (F * nq), f = (e / nq) % F;
            id[j] = (e < n && t < B) ? (int64_t)a.ids[(size_t)t * F + f] : -1;
            if (WV) w[j] = (e < n && t < B) ? a.wts[(size_t)t * F + f] : 0.f;
            if (e < n && t < B && (id[j] < 0 || id[j] >= a.n_rows)) { if (a.err) atomicOr(a.err, 1); id[j] = -1; }
        }
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + 256 * j;
            v[j] = id[j] >= 0 ? *reinterpret_cast<const float4*>(a.table + (size_t)id[j] * rw + 4 * (e % nq)) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (WV && id[j] >= 0) { v[j].x *= w[j]; v[j].y *= w[j]; v[j].z *= w[j]; v[j].w *= w[j]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + 256 * j;
            if (e >= n) continue;
            const int r = e / (F * nq), f = (e / nq) % F, q = e % nq;
            float* d = se + (r * F + f) * SW + 4 * q;
            d[0] = v[j].x; d[1] = v[j].y; d[2] = v[j].z; d[3] = v[j].w;
            if (emb) ipw_store16(a.wt, r_emb, emb, ((size_t)(t0 + r) * FW + f * rw + 4 * q) * 4, v[j]);
        }
    }
    __syncthreads();
    const float bval = *a.b;
    for (int g = threadIdx.x; g < a.D0p / EPL; g += 256) {
        float v[IPW_EX][EPL];
#pragma unroll
        for (int x = 0; x < EPL; ++x) {
            const int c = g * EPL + x;
            int ref = -1;
            float z[IPW_EX];
#pragma unroll
            for (int r = 0; r < IPW_EX; ++r) z[r] = 0.f;
            if (c < FW) {
                const int f = c / rw, l = c - f * rw;
                if (l < K) {
                    ref = f * K + l;
#pragma unroll
                    for (int r = 0; r < IPW_EX; ++r) z[r] = se[(r * F + f) * SW + l];
                }
            } else if (c < CB) {
                int m = c - FW, i = 0;                          // m-th pair (i, j), i < j, row-major
                while (m >= F - 1 - i) { m -= F - 1 - i; ++i; }
                const int j = i + 1 + m;
                ref = F * K + (c - FW);
#pragma unroll
                for (int r = 0; r < IPW_EX; ++r) {
                    const float* pi = se + (r * F + i) * SW;
                    const float* pj = se + (r * F + j) * SW;
                    float s2 = 0.f;
                    for (int l = 0; l < K; ++l) s2 = fmaf(pi[l], pj[l], s2);
                    z[r] = s2;
                }
            } else if (c == CB) {
                ref = a.d0 - 1;
#pragma unroll
                for (int r = 0; r < IPW_EX; ++r) z[r] = bval;
            }
#pragma unroll
            for (int r = 0; r < IPW_EX; ++r) {
                const int t = t0 + r;
                float val = 0.f;
                if (t < B) {
                    if (ref >= 0) val = ip_act(z[r], a.act) * (a.mask ? (float)a.mask[(size_t)t * a.d0 + ref] * a.inv_keep : 1.0f);
                    else if (c == CB + 1) val = 1.0f;
                }
                v[r][x] = val;
            }
        }
#pragma unroll
        for (int r = 0; r < IPW_EX; ++r) {                       // F layout: the EPL columns of an example are one lane slot
            frag fv;
#pragma unroll
            for (int x = 0; x < EPL; ++x) fv[x] = (T)v[r][x];
            ipw_store16(a.wt, r_a0, a0, ft_off<T>(t0 + r, g * EPL, a.D0p) * sizeof(T), fv);
        }
#pragma unroll
        for (int x = 0; x < EPL; ++x)                           // T layout: a column's examples are consecutive k
#pragma unroll
            for (int r = 0; r < IPW_EX; r += 4)
                if (TL) ipw_store4(a.wt, r_a0T, a0T, ft_off<T>(g * EPL + x, t0 + r, a.ldT), v[r][x], v[r + 1][x], v[r + 2][x], v[r + 3][x]);
    }
}
template <typename T, bool WV = false>
static __global__ __launch_bounds__(256) void k_ip_fwd_w(const IpWideArgs a, T* __restrict__ a0, T* __restrict__ a0T, float* __restrict__ emb)
{
    ip_fwd_w_body<T, WV>(a, a0, a0T, emb);
}

// Wide backward: gx'[t][f rw + l] = dz[t][f rw + l] + sum_j dz[t][pair(f, j)] e_j[l] (l < k; pad columns 0), and the per-workgroup
// partial of db.  The embeddings come from emb (the forward's copy); the pair deltas of the 8 examples are staged beside them.
template <bool WV = false>
static __global__ __launch_bounds__(256) void k_ip_bwd_w(const IpWideArgs a, const float* __restrict__ dz, const float* __restrict__ emb,
                                                          float* __restrict__ gxp, float* __restrict__ gb_part)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int F = a.F, K = a.K, rw = a.rw, FW = F * rw, P = a.P, CB = FW + P, D0p = a.D0p;
    float* se = reinterpret_cast<float*>(smem);                 // [IPW_EX][F rw]
    float* sp = se + IPW_EX * FW;                               // [IPW_EX][P]
    float* sw = sp + IPW_EX * P;                                // [IPW_EX][F] value weights (WV only: ipw_bwd_lds)
    const int t0 = blockIdx.x * IPW_EX;
    {
        const int n4 = IPW_EX * FW / 4;                         // the 8 examples' rows are contiguous in emb
        const float4* src = reinterpret_cast<const float4*>(emb + (size_t)t0 * FW);
        for (int e0 = threadIdx.x; e0 < n4; e0 += 256 * 4) {
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int e = e0 + 256 * k; v[k] = e < n4 ? src[e] : make_float4(0.f, 0.f, 0.f, 0.f); }
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int e = e0 + 256 * k; if (e < n4) reinterpret_cast<float4*>(se)[e] = v[k]; }
        }
        for (int e = threadIdx.x; e < IPW_EX * P; e += 256) sp[e] = dz[(size_t)(t0 + e / P) * D0p + FW + e % P];
        if (WV) for (int e = threadIdx.x; e < IPW_EX * F; e += 256) sw[e] = t0 + e / F < a.B ? a.wts[(size_t)t0 * F + e] : 1.0f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < FW; c += 256) {               // a thread owns (field f, lane l) for the 8 examples
        const int f = c / rw, l = c - f * rw;
        float g[IPW_EX];
#pragma unroll
        for (int r = 0; r < IPW_EX; ++r) g[r] = l < K ? dz[(size_t)(t0 + r) * D0p + c] : 0.f;
        if (l < K && P) {
            for (int j = 0; j < F; ++j) {
                if (j == f) continue;
                // pair (i, j), i < j, sits at FW + i (2F - i - 1) / 2 + (j - i - 1)
                const int i0 = f < j ? f : j, j0 = f < j ? j : f, m = i0 * (2 * F - i0 - 1) / 2 + (j0 - i0 - 1);
#pragma unroll
                for (int r = 0; r < IPW_EX; ++r) g[r] = fmaf(sp[r * P + m], se[r * FW + j * rw + l], g[r]);
            }
        }
        if (WV) {
#pragma unroll
            for (int r = 0; r < IPW_EX; ++r) g[r] *= sw[r * F + f];
        }
#pragma unroll
        for (int r = 0; r < IPW_EX; ++r) gxp[(size_t)(t0 + r) * D0p + c] = g[r];
    }
    if (threadIdx.x == 0) { float s = 0.f; for (int r = 0; r < IPW_EX; ++r) s += dz[(size_t)(t0 + r) * D0p + CB]; gb_part[blockIdx.x] = s; }
}

// the bag table's wide sparse-row update (sparse_rows.hip.h) on wide rows: gradient of (example t, field f) at gx'[t][f rw + l]
static __global__ __launch_bounds__(256) void k_ip_scatw1(const ScatArgs sa) { scatw1_body(sa, blockIdx.x); }
static __global__ __launch_bounds__(256) void k_ip_scatw2(const ScatArgs sa)
{
    __shared__ double s_w[1024];
    scatw2_body(sa, blockIdx.x, gridDim.x, s_w);
}

// ------------------------------------------------------------------------------------------
// Many fields (33 .. 64 fields of narrow rows, k <= 16: the reference's own 39 columns): k_ip_fwd's tile of 16 examples x
// (17 F + D0p) floats passes the LDS above 45 fields with pairs (164,736 B at 46, 266,240 B at 64), and where it still fits it
// leaves one workgroup per CU.  These two kernels (each chosen on its own: ip_many_choice) stage the embeddings only, as the wide pair does, on the 16-float slots of
// the narrow table: the forward takes IPM_EX = 8 examples per workgroup (8 x F x 17 floats: 34,816 B at 64 fields, four
// workgroups per CU) and computes every a0 value in registers -- a thread owns EPL consecutive columns of the 8 examples: one
// lane slot of each example's F-layout row and whole lane slots of the T layout.  At 64 fields 2016 of the 3042 used columns
// are pair products, so the column -> (i, j) walk of k_ip_fwd (up to F - 1 trips per column) is a table here (ptab, written at
// create beside ref0: i | j << 8).  The backward takes IPM_BEX = 4 examples: their embeddings and the pair slice of dz
// (4 x (16 F + P) floats: 48,640 B at 64 fields, three workgroups per CU).
// ------------------------------------------------------------------------------------------
constexpr int IPM_EX = 8;       // examples per workgroup of the many-field forward
constexpr int IPM_BEX = 4;      // ... and of the backward
struct IpManyArgs {
    int P; const int32_t* ids; int B, F, K; const float* table16; int64_t n_rows; const float* b;
    const uint8_t* mask; int d0; float inv_keep; int act; int D0p, ldT; int* err;
    const unsigned short* ptab; // [P]: pair n = (i, j), i < j, row-major, as i | j << 8
    bool wt;                    // outputs written through (IPNN_WT=0: plain stores)
    unsigned a0_bytes, emb_bytes;   // sizes of a0 / a0T and of emb: the extent of the write-through stores' buffer resources
    const float* wts;           // value weights [B][F] (read by the WV variants only; NULL: every weight 1)
};
inline size_t ipm_fwd_lds(int F) { return (size_t)IPM_EX * F * (SLOT + 1) * sizeof(float); }
inline size_t ipm_bwd_lds(int F, int P, bool wv) { return (size_t)IPM_BEX * (F * SLOT + P + (wv ? F : 0)) * sizeof(float); }

template <typename T, bool WV, bool TL = true>
__device__ __forceinline__ void ip_fwd_m_body(const IpManyArgs& a, T* __restrict__ a0, T* __restrict__ a0T, float* __restrict__ emb)
{
    typedef typename Traits<T>::frag frag;
    constexpr int EPL = Traits<T>::EPL, SP = SLOT + 1;
    extern __shared__ __align__(16) unsigned char smem[];
    float* se = reinterpret_cast<float*>(smem);                 // [IPM_EX][F][17]: lanes reading slot l of different fields fall on different banks
    const int F = a.F, K = a.K, FS = F * SLOT, FSP = F * SP, CB = FS + a.P, B = a.B;
    const int t0 = blockIdx.x * IPM_EX;
    const __amdgpu_buffer_rsrc_t r_emb = ipw_rsrc(emb, a.emb_bytes), r_a0 = ipw_rsrc(a0, a.a0_bytes), r_a0T = ipw_rsrc(a0T, a.a0_bytes);
    // gather: IPM_EX x F rows of four 16-byte pieces, four in flight per thread; the raw rows also go to emb (the backward's copy)
    const int n = IPM_EX * F * 4;
    for (int e0 = threadIdx.x; e0 < n; e0 += 256 * 4) {
        int64_t id[4];
        float w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + 256 * j, t = t0 + (e >> 2) / F, f = (e >> 2) % F;
            id[j] = (e < n && t < B) ? (int64_t)a.ids[(size_t)t * F + f] : -1;
            if (WV) w[j] = (e < n && t < B) ? a.wts[(size_t)t * F + f] : 0.f;
            if (e < n && t < B && (id[j] < 0 || id[j] >= a.n_rows)) { if (a.err) atomicOr(a.err, 1); id[j] = -1; }
        }
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + 256 * j;
            v[j] = id[j] >= 0 ? *reinterpret_cast<const float4*>(a.table16 + (size_t)id[j] * SLOT + 4 * (e & 3)) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (WV && id[j] >= 0) { v[j].x *= w[j]; v[j].y *= w[j]; v[j].z *= w[j]; v[j].w *= w[j]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + 256 * j;
            if (e >= n) continue;
            const int r = (e >> 2) / F, f = (e >> 2) % F, q = e & 3;
            float* d = se + r * FSP + f * SP + 4 * q;
            d[0] = v[j].x; d[1] = v[j].y; d[2] = v[j].z; d[3] = v[j].w;
            if (emb) ipw_store16(a.wt, r_emb, emb, ((size_t)(t0 + r) * FS + f * SLOT + 4 * q) * 4, v[j]);
        }
    }
    __syncthreads();
    const float bval = *a.b;
    for (int g = threadIdx.x; g < a.D0p / EPL; g += 256) {
        float v[IPM_EX][EPL];
#pragma unroll
        for (int x = 0; x < EPL; ++x) {
            const int c = g * EPL + x;
            int ref = -1, pi = 0, pj = 0;                       // ref: column in the reference's z1 order
            if (c < FS) { if ((c & 15) < K) ref = (c >> 4) * K + (c & 15); }
            else if (c < CB) { const unsigned pr = a.ptab[c - FS]; pi = (int)(pr & 255u); pj = (int)(pr >> 8); ref = F * K + (c - FS); }
            else if (c == CB) ref = a.d0 - 1;
            float mk[IPM_EX];                                   // the column's keep-mask bytes: one round trip, under the products
#pragma unroll
            for (int r = 0; r < IPM_EX; ++r)
                mk[r] = (a.mask && ref >= 0 && t0 + r < B) ? (float)a.mask[(size_t)(t0 + r) * a.d0 + ref] * a.inv_keep : 1.0f;
            float z[IPM_EX];
#pragma unroll
            for (int r = 0; r < IPM_EX; ++r) z[r] = 0.f;
            if (c < FS) {
#pragma unroll
                for (int r = 0; r < IPM_EX; ++r) z[r] = se[r * FSP + (c >> 4) * SP + (c & 15)];
            } else if (c < CB) {
                const float* qi = se + pi * SP;
                const float* qj = se + pj * SP;
                for (int l = 0; l < K; ++l)
#pragma unroll
                    for (int r = 0; r < IPM_EX; ++r) z[r] = fmaf(qi[r * FSP + l], qj[r * FSP + l], z[r]);
            } else if (c == CB) {
#pragma unroll
                for (int r = 0; r < IPM_EX; ++r) z[r] = bval;
            }
#pragma unroll
            for (int r = 0; r < IPM_EX; ++r) {
                float val = 0.f;
                if (t0 + r < B) {
                    if (ref >= 0) val = ip_act(z[r], a.act) * mk[r];
                    else if (c == CB + 1) val = 1.0f;
                }
                v[r][x] = val;
            }
        }
#pragma unroll
        for (int r = 0; r < IPM_EX; ++r) {                       // F layout: the EPL columns of an example are one lane slot
            frag fv;
#pragma unroll
            for (int x = 0; x < EPL; ++x) fv[x] = (T)v[r][x];
            ipw_store16(a.wt, r_a0, a0, ft_off<T>(t0 + r, g * EPL, a.D0p) * sizeof(T), fv);
        }
#pragma unroll
        for (int x = 0; x < EPL; ++x)                           // T layout: a column's examples are consecutive k
#pragma unroll
            for (int r = 0; r < IPM_EX; r += 4)
                if (TL) ipw_store4(a.wt, r_a0T, a0T, ft_off<T>(g * EPL + x, t0 + r, a.ldT), v[r][x], v[r + 1][x], v[r + 2][x], v[r + 3][x]);
    }
}
template <typename T, bool WV = false>
static __global__ __launch_bounds__(256) void k_ip_fwd_m(const IpManyArgs a, T* __restrict__ a0, T* __restrict__ a0T, float* __restrict__ emb)
{
    ip_fwd_m_body<T, WV>(a, a0, a0T, emb);
}

// Many-field backward: gx'[t][16 f + l] = dz[t][16 f + l] + sum_{j != f} dz[t][pair(f, j)] e_j[l] (l < k; pad columns 0) and the
// per-workgroup partial of db (one per IPM_BEX examples).  The embeddings come from emb (the forward's copy).  A wave holds four
// fields x 16 slots: its read of e_j[l] is 16 addresses broadcast to the four fields, its read of the pair delta four addresses.
// (the body of k_ip_bwd_m and of its group form k_ip_bwd_m_g)
template <bool WV>
__device__ __forceinline__ void ip_bwd_m_body(const IpManyArgs& a, const float* __restrict__ dz, const float* __restrict__ emb,
                                              float* __restrict__ gxp, float* __restrict__ gb_part)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int F = a.F, K = a.K, FS = F * SLOT, P = a.P, CB = FS + P, D0p = a.D0p;
    float* se = reinterpret_cast<float*>(smem);                 // [IPM_BEX][16 F]
    float* sp = se + IPM_BEX * FS;                              // [IPM_BEX][P]
    float* sw = sp + IPM_BEX * P;                               // [IPM_BEX][F] value weights (WV only: ipm_bwd_lds)
    const int t0 = blockIdx.x * IPM_BEX;
    {
        const int n4 = IPM_BEX * FS / 4;                        // the examples' rows are contiguous in emb
        const float4* src = reinterpret_cast<const float4*>(emb + (size_t)t0 * FS);
        for (int e0 = threadIdx.x; e0 < n4; e0 += 256 * 4) {
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int e = e0 + 256 * k; v[k] = e < n4 ? src[e] : make_float4(0.f, 0.f, 0.f, 0.f); }
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int e = e0 + 256 * k; if (e < n4) reinterpret_cast<float4*>(se)[e] = v[k]; }
        }
        // the pair slice of each example starts at column 16 F of a row of D0p floats: both multiples of 4, 16-byte pieces up to
        // the last whole one, the rest one float at a time
        const int p4 = P >> 2;
        for (int e = threadIdx.x; e < IPM_BEX * p4; e += 256) {
            const int r = e / p4, q = e - r * p4;
            const float4 v = *reinterpret_cast<const float4*>(dz + (size_t)(t0 + r) * D0p + FS + 4 * q);
            float* d = sp + r * P + 4 * q;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        const int rest = P & 3;
        if ((int)threadIdx.x < IPM_BEX * rest) {
            const int r = threadIdx.x / rest, q = 4 * p4 + threadIdx.x % rest;
            sp[r * P + q] = dz[(size_t)(t0 + r) * D0p + FS + q];
        }
        if (WV) for (int e = threadIdx.x; e < IPM_BEX * F; e += 256) sw[e] = t0 + e / F < a.B ? a.wts[(size_t)t0 * F + e] : 1.0f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < FS; c += 256) {               // a thread owns (field f, slot l) for the IPM_BEX examples
        const int f = c >> 4, l = c & 15;
        float g[IPM_BEX];
#pragma unroll
        for (int r = 0; r < IPM_BEX; ++r) g[r] = l < K ? dz[(size_t)(t0 + r) * D0p + c] : 0.f;
        if (l < K && P) {
            // pair (i, j), i < j, sits at i (2F - i - 1) / 2 + (j - i - 1): partners below f walk down the column of f, partners
            // above it along its row
            for (int j = 0; j < f; ++j) {
                const int m = j * (2 * F - j - 1) / 2 + (f - j - 1);
#pragma unroll
                for (int r = 0; r < IPM_BEX; ++r) g[r] = fmaf(sp[r * P + m], se[r * FS + j * SLOT + l], g[r]);
            }
            const int m0 = f * (2 * F - f - 1) / 2 - f - 1;
            for (int j = f + 1; j < F; ++j) {
#pragma unroll
                for (int r = 0; r < IPM_BEX; ++r) g[r] = fmaf(sp[r * P + m0 + j], se[r * FS + j * SLOT + l], g[r]);
            }
        }
        if (WV) {
#pragma unroll
            for (int r = 0; r < IPM_BEX; ++r) g[r] *= sw[r * F + f];
        }
#pragma unroll
        for (int r = 0; r < IPM_BEX; ++r) gxp[(size_t)(t0 + r) * D0p + c] = g[r];
    }
    if (threadIdx.x == 0) { float s = 0.f; for (int r = 0; r < IPM_BEX; ++r) s += dz[(size_t)(t0 + r) * D0p + CB]; gb_part[blockIdx.x] = s; }
}
template <bool WV = false>
static __global__ __launch_bounds__(256) void k_ip_bwd_m(const IpManyArgs a, const float* __restrict__ dz, const float* __restrict__ emb,
                                                          float* __restrict__ gxp, float* __restrict__ gb_part)
{
    ip_bwd_m_body<WV>(a, dz, emb, gxp, gb_part);
}

}  // namespace
