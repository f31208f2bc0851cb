// fm_kernels.hip.h -- the kernels of factorisation-machine pre-training (gfx950 only): the forwards of both layouts with their
// merge-beside forms, the bias / loss tail beside level 2 of the sparse-row update, and the passes over the table.  A part of
// the unit fm_api.hip, which alone includes it.
//   FmArgs                              one forward (+ gradients) as arguments
//   fm_body<NF, WV>                     narrow rows (k <= 16): k_fm, k_fm_merge_fwd (the rank merge of the batch's sort beside it)
//   fm_wide_body<L, NC, WV>             wide rows (k >= 17), L = 16 or 32 lanes an example: k_fm_wide, k_fm_wide_merge_fwd
//   FmBiasOpt, fm_opt_step, fm_tail_body  the bias and the loss: k_fm_scat2_tail, k_fm_scat2s_tail (with k_fm_scat1s: shared
//                                       rows), k_fm_scatw2_tail (with k_fm_scatw1: wide rows)
//   k_fm_count_marks, k_fm_rescale, k_fm_fill, k_fm_opt_pass<DENSE_G>
// The group forms of the forwards and of the step are in fm_group_kernels.hip.h; which instantiation a handle takes is the
// plan's business (fm_plan.h) and is dispatched in one place (fm_ladder, fm_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fm_hip.h"
#include "sparse_rows.hip.h"
#include "optim.hip.h"

namespace {
using namespace fnn;

// 16 lanes per example: lane f owns fields f, f + 16, .. (NF = ceil(F / 16) of them; NF = 1 up to 16 fields, lane = field) and
// loads their 64-byte rows, sums them in registers, and the field sums S_l = sum_f v_f[l] are 4-step shuffle reductions inside
// the 16-lane group.
struct FmArgs {
    const int32_t* ids; const float* y; int B, F, K; const float* table16; int64_t n_rows; const float* b;
    float scale, dscale; int train; float* gxp; int K1p; float* p_out; float* loss_t; float* gb_part; int* err;
    bool wt;                   // gx' written through (see store4_wt in fnn_kernels.hip.h)
    int* stamp; int step;      // Adam / FTRL: stamp[row] = step for every row the batch touches (null: not kept)
    int rw;                    // wide rows (fm_wide_body): the row stride in floats, a multiple of 4; gx' is [t][F][rw]
    const float* wts;          // value weights [B, F] beside ids (the WV = true kernels), or null: every value is 1
};

// store16_sel and the two wait states gfx950 needs before a VALU instruction may overwrite the data VGPRs of a store wider than 8
// bytes: the compiler provides them after its own stores, not after store16_wt's inline assembly.  With several fields per lane the
// next field's gradients are computed into the registers the previous store reads (NF = 1 stores last: store16_sel as it was;
// every weighted kernel, WV = true, stores through this one).
__device__ __forceinline__ void store16_sel_ws(const bool wt, float* p, const float4 v)
{
    u32x4 w; __builtin_memcpy(&w, &v, 16);
    if (wt) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(p), "v"(w) : "memory");
    else *reinterpret_cast<u32x4*>(p) = w;
}
// WV: value weights (python/FM.py:24-29's sp_wt_hldr).  x = wts[t][fld] is loaded beside the id, the row enters as e = x * row, and
// lin, S and sq follow from e as they did from the row; d yhat / d w_f = x, d yhat / d v_f[l] = x (S_l - e_f[l]).  The weight of
// an absent field or of a padding example is replaced by 0 (its row by zeros), so that no value there, NaN included, reaches e.
template <int NF, bool WV>
__device__ __forceinline__ void fm_body(const FmArgs& a, const int blk, float* s_gb)
{
    const int tid = threadIdx.x, f = tid & 15, grp = tid >> 4;
    const int t = blk * 16 + grp;
    int64_t id[NF];
    float x[NF];
#pragma unroll
    for (int n = 0; n < NF; ++n) {                          // every id first: the row loads below do not wait behind a stamp
        const int fld = f + 16 * n;
        id[n] = -1;
        x[n] = 0.f;
        if (t < a.B && fld < a.F) {
            id[n] = a.ids[(size_t)t * a.F + fld];
            if (WV) x[n] = a.wts[(size_t)t * a.F + fld];    // in the id's round trip
            if (id[n] < -1 || id[n] >= a.n_rows) { atomicOr(a.err, 1); id[n] = -1; }
            if (a.stamp && id[n] >= 0) a.stamp[id[n]] = a.step;
            if (WV && id[n] < 0) x[n] = 0.f;
        }
    }
    float r[NF][16];
#pragma unroll
    for (int n = 0; n < NF; ++n) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (id[n] >= 0) v = *reinterpret_cast<const float4*>(a.table16 + (size_t)id[n] * SLOT + 4 * q);
            r[n][4 * q] = v.x * a.scale; r[n][4 * q + 1] = v.y * a.scale; r[n][4 * q + 2] = v.z * a.scale; r[n][4 * q + 3] = v.w * a.scale;
            if (WV) { r[n][4 * q] *= x[n]; r[n][4 * q + 1] *= x[n]; r[n][4 * q + 2] *= x[n]; r[n][4 * q + 3] *= x[n]; }
        }
    }
    // yhat = b + sum_f w_f + 1/2 (sum_l S_l^2 - sum_f sum_l v_f[l]^2)                     (:56-63)
    float lin = r[0][0], sq = 0.f, S[16];
#pragma unroll
    for (int l = 1; l < 16; ++l) { S[l] = r[0][l]; sq = fmaf(r[0][l], r[0][l], sq); }
#pragma unroll
    for (int n = 1; n < NF; ++n) {                          // the lane's further fields, in field order
        lin += r[n][0];
#pragma unroll
        for (int l = 1; l < 16; ++l) { S[l] += r[n][l]; sq = fmaf(r[n][l], r[n][l], sq); }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        lin += __shfl_xor(lin, o, 16); sq += __shfl_xor(sq, o, 16);
#pragma unroll
        for (int l = 1; l < 16; ++l) S[l] += __shfl_xor(S[l], o, 16);
    }
    float ss = 0.f;
#pragma unroll
    for (int l = 1; l < 16; ++l) ss = fmaf(S[l], S[l], ss);
    const float z = *a.b + lin + 0.5f * (ss - sq);
    const float p = 1.0f / (1.0f + expf(-z));
    float delta = 0.f;
    if (t < a.B) {
        if (a.p_out && f == 0) a.p_out[t] = p;
        if (a.train) {
            const float yy = a.y[t];
            delta = (p - yy) * a.dscale;                         // dscale = 1 (sum) or 1/B (mean)
            if (f == 0) a.loss_t[t] = fmaxf(z, 0.f) - z * yy + log1pf(expf(-fabsf(z)));
        }
    } else if (a.train && f == 0) a.loss_t[t] = 0.f;
    if (!a.train) return;
    // d yhat / d w_f = x_f ; d yhat / d v_f[l] = x_f (S_l - e_f[l])   (WV = false: x = 1)
#pragma unroll
    for (int n = 0; n < NF; ++n) {
        const int fld = f + 16 * n;
        const float dx = WV ? delta * x[n] : delta;
        float g[16];
        g[0] = (id[n] >= 0) ? dx : 0.f;
#pragma unroll
        for (int l = 1; l < 16; ++l) g[l] = (id[n] >= 0 && l < a.K) ? dx * (S[l] - r[n][l]) : 0.f;
        float* out = a.gxp + (size_t)t * a.K1p + fld * SLOT;    // K1p = rup(F, 16) * SLOT
        if (fld < a.F) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {                   // (written through: FM_WT=0 for plain stores)
                const float4 g4 = make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
                if (NF == 1 && !WV) store16_sel(a.wt, out + 4 * q, g4);
                else store16_sel_ws(a.wt, out + 4 * q, g4);
            }
        }
    }
    if (f == 0) s_gb[grp] = delta;
    __syncthreads();
    if (tid == 0) { float s = 0.f; for (int i = 0; i < 16; ++i) s += s_gb[i]; a.gb_part[blk] = s; }
}
template <int NF, bool WV>
__global__ __launch_bounds__(256) void k_fm(const FmArgs a)
{
    __shared__ float s_gb[16];
    fm_body<NF, WV>(a, blockIdx.x, s_gb);
}
// Wide rows (k >= 17): L lanes per example (16 while the row's rw / 4 float4 pieces fit, else 32); lane q owns columns 4q..4q+3
// of every field's row and issues its example's row loads 16 fields at a time, so that S_l = sum_f v_f[l] is a register sum and
// only the example's scalar b + lin + 1/2 sum_l (S_l^2 - sum_f v_f[l]^2) crosses lanes.  Lane q reads, checks and stamps the ids
// of fields q, q + L, .. (< F).  gx'[t][f] = delta * [1 | S - v_f], zero in the padding columns (>= K); absent fields are not
// written (no record points at them).  More than 16 fields (NC = ceil(F / 16) chunks of 16): a rolled first pass sums every
// chunk, the second reloads each chunk's rows and writes its gradients (holding the last chunk across the passes cost 30-40
// VGPRs and an occupancy step).  NC = 1, up to 16 fields: the gradients from the rows still in registers, nothing reloaded.
// WV (value weights, as in fm_body): lane q keeps the weights of its fields beside their ids (0 where the id is absent), a chunk's
// weights x[16] are shuffled out with its ids, and the rows enter as e = (scale x) row in BOTH passes -- the second pass has to
// reproduce the first pass's e bit for bit; x[] lives across one chunk only.
template <int L, int NR, bool WV>
__device__ __forceinline__ void fm_wide_chunk(const FmArgs& a, const int (&mine)[NR], const float (&minex)[NR], const int c, const int q,
                                              const int nq, int (&id)[16], float (&x)[16], float4 (&v)[16])
{
    // fields 16 c .. 16 c + 15 lie in one round of ids (L = 16 or 32): round 16 c / L, lanes 16 c % L + f
    int m = mine[0];
    float mx = minex[0];
#pragma unroll
    for (int r = 1; r < NR; ++r) { m = (r == 16 * c / L) ? mine[r] : m; if (WV) mx = (r == 16 * c / L) ? minex[r] : mx; }
#pragma unroll
    for (int f = 0; f < 16; ++f) {
        id[f] = __shfl(m, 16 * c % L + f, L);             // -1 for fields >= F
        if (WV) x[f] = __shfl(mx, 16 * c % L + f, L);     // 0 where the id is -1
        v[f] = (id[f] >= 0 && q < nq) ? *reinterpret_cast<const float4*>(a.table16 + (size_t)id[f] * a.rw + 4 * q)
                                      : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
template <bool WV>
__device__ __forceinline__ void fm_wide_grads(const FmArgs& a, float* out, const int c, const int (&id)[16], const float (&x)[16],
                                              const float4 (&v)[16], const float4 S, const float delta)
{
#pragma unroll
    for (int f = 0; f < 16; ++f) {
        if (id[f] < 0) continue;
        const float dx = WV ? delta * x[f] : delta;
        const float4 g = make_float4(c == 0 ? dx : (c < a.K ? dx * (S.x - v[f].x) : 0.f),
                                     c + 1 < a.K ? dx * (S.y - v[f].y) : 0.f,
                                     c + 2 < a.K ? dx * (S.z - v[f].z) : 0.f,
                                     c + 3 < a.K ? dx * (S.w - v[f].w) : 0.f);
        if (WV) store16_sel_ws(a.wt, out + (size_t)f * a.rw, g);
        else store16_sel(a.wt, out + (size_t)f * a.rw, g);
    }
}
template <int L, int NC, bool WV>
__device__ __forceinline__ void fm_wide_body(const FmArgs& a, const int blk, float* s_gb /*[256 / L]*/)
{
    constexpr int EPB = 256 / L;                          // examples per workgroup
    constexpr int NR = (16 * NC + L - 1) / L;             // id rounds: lane q holds the ids of fields q, q + L, ..
    const int tid = threadIdx.x, q = tid % L, grp = tid / L, nq = a.rw >> 2;
    const int t = blk * EPB + grp;
    int mine[NR];
    float minex[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int fld = q + r * L;
        mine[r] = -1;
        minex[r] = 0.f;
        if (t < a.B && fld < a.F) {
            const int64_t id = a.ids[(size_t)t * a.F + fld];
            float w = 0.f;
            if (WV) w = a.wts[(size_t)t * a.F + fld];       // in the id's round trip
            if (id < -1 || id >= a.n_rows) atomicOr(a.err, 1);
            else mine[r] = (int)id;
            if (a.stamp && mine[r] >= 0) a.stamp[mine[r]] = a.step;
            if (WV && mine[r] >= 0) minex[r] = w;
        }
    }
    int id[16];
    float x[16];
    float4 v[16];
    float lin = 0.f;
    float4 S = make_float4(0.f, 0.f, 0.f, 0.f), sq = S;
#pragma unroll 1
    for (int c = 0; c < NC; ++c) {                        // rolled: one chunk's 16 rows in registers at a time
        fm_wide_chunk<L, NR, WV>(a, mine, minex, c, q, nq, id, x, v);
#pragma unroll
        for (int f = 0; f < 16; ++f) {
            const float s = WV ? a.scale * x[f] : a.scale;    // e = (scale x) row
            v[f].x *= s; v[f].y *= s; v[f].z *= s; v[f].w *= s;
            if (q == 0) { lin += v[f].x; v[f].x = 0.f; }      // column 0 is w_f
            S.x += v[f].x; S.y += v[f].y; S.z += v[f].z; S.w += v[f].w;
            sq.x = fmaf(v[f].x, v[f].x, sq.x); sq.y = fmaf(v[f].y, v[f].y, sq.y);
            sq.z = fmaf(v[f].z, v[f].z, sq.z); sq.w = fmaf(v[f].w, v[f].w, sq.w);
        }
    }
    // yhat = b + sum_f w_f + 1/2 (sum_l S_l^2 - sum_f sum_l v_f[l]^2)                     (:56-63)
    float part = lin + 0.5f * ((fmaf(S.x, S.x, -sq.x) + fmaf(S.y, S.y, -sq.y)) + (fmaf(S.z, S.z, -sq.z) + fmaf(S.w, S.w, -sq.w)));
#pragma unroll
    for (int o = 1; o < L; o <<= 1) part += __shfl_xor(part, o, L);
    const float z = *a.b + part;
    const float p = 1.0f / (1.0f + expf(-z));
    float delta = 0.f;
    if (t < a.B) {
        if (a.p_out && q == 0) a.p_out[t] = p;
        if (a.train) {
            const float yy = a.y[t];
            delta = (p - yy) * a.dscale;                         // dscale = 1 (sum) or 1/B (mean)
            if (q == 0) a.loss_t[t] = fmaxf(z, 0.f) - z * yy + log1pf(expf(-fabsf(z)));
        }
    } else if (a.train && q == 0) a.loss_t[t] = 0.f;
    if (!a.train) return;
    // d yhat / d w_f = x_f ; d yhat / d v_f[l] = x_f (S_l - e_f[l])   (WV = false: x = 1)
    float* out = a.gxp + (size_t)t * a.K1p + 4 * q;
    if (NC == 1) {                                        // up to 16 fields: the rows are still in registers
        if (q < nq) fm_wide_grads<WV>(a, out, 4 * q, id, x, v, S, delta);
    } else {
#pragma unroll 1
        for (int c = 0; c < NC; ++c) {                    // every chunk's rows again (the shuffles with the whole group)
            fm_wide_chunk<L, NR, WV>(a, mine, minex, c, q, nq, id, x, v);
#pragma unroll
            for (int f = 0; f < 16; ++f) {
                const float s = WV ? a.scale * x[f] : a.scale;
                v[f].x *= s; v[f].y *= s; v[f].z *= s; v[f].w *= s;
            }
            if (q < nq) fm_wide_grads<WV>(a, out + (size_t)(16 * c) * a.rw, 4 * q, id, x, v, S, delta);
        }
    }
    if (q == 0) s_gb[grp] = delta;
    __syncthreads();
    if (tid == 0) { float s = 0.f; for (int i = 0; i < EPB; ++i) s += s_gb[i]; a.gb_part[blk] = s; }
}
template <int L, int NC, bool WV>
__global__ __launch_bounds__(256) void k_fm_wide(const FmArgs a)
{
    __shared__ float s_gb[256 / L];
    fm_wide_body<L, NC, WV>(a, blockIdx.x, s_gb);
}
template <typename KT, int L, int NC, bool WV>
__global__ __launch_bounds__(256) void k_fm_wide_merge_fwd(const SortArgs so, const FmArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ float s_gb[256 / L];
    if ((int)blockIdx.x < so.nblk) { sortB_body<KT>(so, blockIdx.x, smem); return; }
    fm_wide_body<L, NC, WV>(a, (int)blockIdx.x - so.nblk, s_gb);
}

// A training step is four launches: run sorts of the batch's (row, t) keys; their rank merge BESIDE the forward + gradients
// (both need only the ids: the merge takes 16 F workgroups, the examples the rest); level-1 sparse-row update; level-2 update
// BESIDE the bias / loss tail.  As six launches in a row (sort, sort, forward, scatter, scatter, tail) the step took 49.6 us.
template <typename KT, int NF, bool WV>
__global__ __launch_bounds__(256) void k_fm_merge_fwd(const SortArgs so, const FmArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ float s_gb[16];
    if ((int)blockIdx.x < so.nblk) { sortB_body<KT>(so, blockIdx.x, smem); return; }
    fm_body<NF, WV>(a, (int)blockIdx.x - so.nblk, s_gb);
}

// The bias under Adam / FTRL: the state beside it (sb [2]) and this step's learning rate (Adam: lr_t).  opt = 0: SGD.
struct FmBiasOpt { int opt; float* sb; float lr, b1, b2, eps; };
__device__ __forceinline__ float fm_opt_step(int opt, float w, float g, float& s0, float& s1, float lr, float b1, float b2, float eps) {
    return opt == FM_OPT_FTRL ? ftrl_step(w, g, s0, s1, lr) : adam_step(w, g, s0, s1, lr, b1, b2, eps);
}

// b <- b (1 - lr lambda) - lr sum(delta) (Adam / FTRL: the optimiser on g = sum(delta) + lambda b); loss sum (fixed-shape tree)
__device__ __forceinline__ void fm_tail_body(float* b, const float* gb_part, int n, float lr, float lambda, const float* loss_t, int Ba, float lscale,
                                             float* loss_out, float* sl, const FmBiasOpt& bo)
{   // both sums as 256 strided partial sums and a fixed-shape tree (one thread walking the n partials paid a memory round trip
    // per element: 19 us for 256 of them)
    float v = strided_sum256(gb_part, n);
    sl[threadIdx.x] = v; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) sl[threadIdx.x] += sl[threadIdx.x + o]; __syncthreads(); }
    const float gsum = sl[0];
    __syncthreads();
    v = strided_sum256(loss_t, Ba);
    sl[threadIdx.x] = v; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) sl[threadIdx.x] += sl[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) {
        if (bo.opt) *b = fm_opt_step(bo.opt, *b, gsum + lambda * *b, bo.sb[0], bo.sb[1], bo.lr, bo.b1, bo.b2, bo.eps);
        else *b = *b * (1.0f - lr * lambda) - lr * gsum;
        *loss_out = sl[0] * lscale;
    }
}
__global__ __launch_bounds__(256) void k_fm_scat2_tail(const ScatArgs sa, float* b, const float* gb_part, int n, float lr, float lambda,
                                                       const float* loss_t, int Ba, float lscale, float* loss_out, const FmBiasOpt bo)
{
    __shared__ double s_sum[16][16];
    if (blockIdx.x == 0) { fm_tail_body(b, gb_part, n, lr, lambda, loss_t, Ba, lscale, loss_out, reinterpret_cast<float*>(&s_sum[0][0]), bo); return; }
    if (sa.form2 == SCAT2_WAVE) scat2w_body(sa, (int)blockIdx.x - 1, (int)gridDim.x - 1);
    else scat2_body(sa, (int)blockIdx.x - 1, (int)gridDim.x - 1, s_sum);
}
// Shared rows (fm_set_shared_rows): the half-chunk level 1 and the wave-per-segment level 2 in their SHARED forms, whatever
// FNN_SCAT1_FORM / FNN_SCAT2_FORM say -- rows the rank merge marked (SortArgs::tag_shared) take float atomics, the others the
// stores of k_scat1 / k_fm_scat2_tail.  FM only: the FNN step's and the inner-product family's columns are fields.
__global__ __launch_bounds__(256) void k_fm_scat1s(const ScatArgs sa) { scat1h_form<true>(sa, blockIdx.x); }
__global__ __launch_bounds__(256) void k_fm_scat2s_tail(const ScatArgs sa, float* b, const float* gb_part, int n, float lr, float lambda,
                                                        const float* loss_t, int Ba, float lscale, float* loss_out, const FmBiasOpt bo)
{
    __shared__ float s_l[256];
    if (blockIdx.x == 0) { fm_tail_body(b, gb_part, n, lr, lambda, loss_t, Ba, lscale, loss_out, s_l, bo); return; }
    scat2w_form<true>(sa, (int)blockIdx.x - 1, (int)gridDim.x - 1);
}
// fm_count_shared_rows: the rows the last step's rank merge marked
__global__ __launch_bounds__(256) void k_fm_count_marks(const int* __restrict__ tag_shared, int64_t n_rows, int stamp, unsigned long long* out)
{
    __shared__ int s_c[256];
    int c = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_rows; i += (int64_t)gridDim.x * 256) c += tag_shared[i] == stamp;
    s_c[threadIdx.x] = c; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) s_c[threadIdx.x] += s_c[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0 && s_c[0]) atomicAdd(out, (unsigned long long)s_c[0]);
}
// the same for wide rows: level 1 on its own, level 2 (8 KiB of LDS) beside the tail
__global__ __launch_bounds__(256) void k_fm_scatw1(const ScatArgs sa) { scatw1_body(sa, blockIdx.x); }
__global__ __launch_bounds__(256) void k_fm_scatw2_tail(const ScatArgs sa, float* b, const float* gb_part, int n, float lr, float lambda,
                                                        const float* loss_t, int Ba, float lscale, float* loss_out, const FmBiasOpt bo)
{
    __shared__ double s_w[1024];
    if (blockIdx.x == 0) { fm_tail_body(b, gb_part, n, lr, lambda, loss_t, Ba, lscale, loss_out, reinterpret_cast<float*>(s_w), bo); return; }
    scatw2_body(sa, (int)blockIdx.x - 1, (int)gridDim.x - 1, s_w);
}

__global__ void k_fm_rescale(float* table16, size_t n, float s)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) table16[i] *= s;
}

__global__ void k_fm_fill(float* p, size_t n, float v)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// Adam / FTRL on the table: the L2 term makes TensorFlow's gradient DENSE, so every live element (row < n_rows, column < K)
// moves each step: g = G + lambda w, the optimiser, w and both state values written back.  The state is compact [n_rows, K]
// (s0 / s1 rounded up to a multiple of 4 floats): a thread owns 4 consecutive elements of it -- one 16-byte access per state
// array -- and the matching 4 table / G elements at their padded-row addresses (row stride rw); padding columns are never touched.
// G (the batch's per-row gradient sums, padded rows) is read and cleared only where it was written: DENSE_G = false reads a
// row's G when stamp[row] == step (the rows this step's forward touched); DENSE_G = true reads and clears every element of G.
template <bool DENSE_G>
__global__ __launch_bounds__(256) void k_fm_opt_pass(float* __restrict__ table16, float* __restrict__ G, const int* __restrict__ stamp, int step,
                                                     float* __restrict__ s0, float* __restrict__ s1, size_t nk, int K, int rw, float lambda,
                                                     int opt, float lr, float b1, float b2, float eps)
{
    const size_t e0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e0 >= nk) return;
    size_t row = e0 / K;
    int c = (int)(e0 - row * K);
    const float4 m4 = *reinterpret_cast<const float4*>(s0 + e0), v4 = *reinterpret_cast<const float4*>(s1 + e0);
    float m[4] = {m4.x, m4.y, m4.z, m4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w}, w[4], g[4];
    size_t off[4];
    bool live[4], hit[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                      // every load first, then the arithmetic, then the stores
        live[j] = e0 + j < nk;
        off[j] = row * rw + c;
        w[j] = live[j] ? table16[off[j]] : 0.f;
        hit[j] = live[j] && (DENSE_G || stamp[row] == step);
        g[j] = hit[j] ? G[off[j]] : 0.f;
        if (++c == K) { c = 0; ++row; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (!live[j]) continue;
        w[j] = fm_opt_step(opt, w[j], g[j] + lambda * w[j], m[j], v[j], lr, b1, b2, eps);
        table16[off[j]] = w[j];
        if (hit[j]) G[off[j]] = 0.f;
    }
    *reinterpret_cast<float4*>(s0 + e0) = make_float4(m[0], m[1], m[2], m[3]);
    *reinterpret_cast<float4*>(s1 + e0) = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace
