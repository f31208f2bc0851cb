// fm_api.hip -- factorisation-machine pre-training on gfx950 behind include/fm_hip.h (row N3):
// python/FM.py:55-64 (factorization), :36-41 (loss) and plain SGD, on the FNN path's building
// blocks: padded 64-byte rows, the split sort + two-level segmented sparse-row update.  Adam and
// FTRL (python/tf_util.py:15-24): the same sorted sums into a zeroed gradient store, then one
// streaming pass over the live elements of the table and its compact state (k_fm_opt_pass).
// Wide rows (k >= 17, ranks 16..127: the reference's FM50 / FM100): rows of rup(k, 4) floats, the forward of fm_wide_body and
// the bag table's wide sparse-row update (scatw1_body / scatw2_body); the sort, the tail and the optimiser pass are shared.
// 1..64 fields on both layouts: the forwards take 16 fields at a time (fm_body<NF>, fm_wide_body<L, NC>; one instantiation per
// 16 fields, the first being the 16-field kernels); the sort and both sparse-row updates are the FNN step's, sized by F.
// Several models on one test feed (fm_predict_multi, fm_eval_multi): the same forward bodies, the arguments of each model read from
// a device array (k_fm_multi, k_fm_wide_multi), and the metric pass of metrics.hip with a model dimension (metrics_multi).
// Several models, one mini-batch step (fm_train_step_multi): the models that agree in n_rows and the shared-rows mode share the
// batch's run sort and rank merge, and the step's bodies run once per layout present with the model as a grid dimension (k_fm_step_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fm_hip.h"
#include "../../include/fnn_hip.h"
#include "sparse_rows.hip.h"
#include "metrics.hip.h"
#include "optim.hip.h"
#include "fm_online.hip.h"
#include "arg_ring.h"
#include "group_call.h"

using namespace fnn;

namespace {

thread_local std::string g_fm_err;
inline int rup(int x, int m) { return (x + m - 1) / m * m; }

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

// Predictions of several models on one feed (fm_predict_multi, fm_eval_multi): the forward bodies above with train = 0, the
// arguments of model m read from a device array instead of the kernel's own (k_fm_online_multi's way), so p is bit for bit what
// k_fm / k_fm_wide write for that model: an example's p depends on its own lines and rows only, not on the batch around it.
// One launch per layout class present in a call (narrow; wide at 16 lanes an example; wide at 32), so that the narrow models do
// not run at the wide bodies' register count: cls[0 .. nm) lists the class's models as indices into args.  The grid is the
// (model, example tile) pairs flattened over x and y; model_fast: neighbouring workgroups take the same tile of different
// models (the feed's lines are shared, the tables are not), else a model's tiles are neighbours (one table at a time).
struct EvalArg { FmArgs a; int cls; };
__device__ __forceinline__ bool eval_pick(const EvalArg* __restrict__ args, const int first, const int nm, const int64_t tiles,
                                          const int model_fast, int& m, int& tile)
{
    const int64_t lin = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (lin >= tiles * nm) return false;
    const int64_t j = model_fast ? lin % nm : lin / tiles;
    tile = (int)(model_fast ? lin / nm : lin % tiles);
    m = args[first + j].cls;
    return true;
}
template <int NF, bool WV>
__global__ __launch_bounds__(256) void k_fm_multi(const EvalArg* __restrict__ args, const int first, const int nm, const int64_t tiles,
                                                  const int model_fast)
{
    __shared__ float s_gb[16];
    int m, tile;
    if (!eval_pick(args, first, nm, tiles, model_fast, m, tile)) return;
    const FmArgs a = args[m].a;
    fm_body<NF, WV>(a, tile, s_gb);
}
template <int L, int NC, bool WV>
__global__ __launch_bounds__(256) void k_fm_wide_multi(const EvalArg* __restrict__ args, const int first, const int nm, const int64_t tiles,
                                                       const int model_fast)
{
    __shared__ float s_gb[256 / L];
    int m, tile;
    if (!eval_pick(args, first, nm, tiles, model_fast, m, tile)) return;
    const FmArgs a = args[m].a;
    fm_wide_body<L, NC, WV>(a, tile, s_gb);
}
// fm_eval_multi: the range flags of a group's models, read and then cleared where set (fm_sync's rule); one workgroup, so that a
// handle listed twice shows its flag in both places before either clears it.
__global__ __launch_bounds__(256) void k_fm_eval_flags(const EvalArg* __restrict__ args, const int n, int* __restrict__ flags)
{
    for (int i = threadIdx.x; i < n; i += 256) flags[i] = *static_cast<volatile int*>(args[i].a.err);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) if (flags[i]) *args[i].a.err = 0;
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

// One mini-batch step of several models on one feed (fm_train_step_multi): the bodies above, the arguments of model m read from a
// device array (k_fm_multi's way), the model a grid dimension.  The grouping -- run sort and rank merge -- depends on the ids,
// n_rows and the shared-rows mode only, so the models that agree in those (a grouping CLASS) share one: every model's update reads
// the class's rec (and shared-row marks) with its own part / owners / owner_cnt, gx', table and scale.
//   launch 1  the run sort of a class (k_sortA), as the solo step's
//   launch 2  k_fm_step_fwd / k_fm_step_fwd_wide, one per layout present: the classes' rank merges (16 F workgroups each, in the
//             first such launch) beside the forward + gradients of every (model, example tile) of the layout
//   launch 3  k_fm_step_scat1 / k_fm_step_scatw1: level 1, grid (workgroups of the largest model, models)
//   launch 4  k_fm_step_scat2_tail / k_fm_step_scatw2_tail: per model the bias / loss tail and 256 level-2 workgroups
// The narrow rows take the half-chunk level 1 and the wave level 2 whatever FNN_SCAT1_FORM / FNN_SCAT2_FORM say: every form
// gives the same bits (tests/test_gpu_scat1_half.py, test_gpu_scat2_forms.py).
struct StepTail { float* b; const float* gb_part; int n; float lr, lambda; const float* loss_t; int Ba; float lscale; float* loss_out; FmBiasOpt bo; };
struct StepPack { float loss; int flag; };
struct StepArg {
    FmArgs a; ScatArgs sa; StepTail t;
    // a shared-rows model that is not its class's first: the class's marks (sa.tag_shared, sa.stamp) are copied into its own
    // array under its own stamp (null: nothing to copy) -- what fm_count_shared_rows scans for this handle
    int* own_marks; int own_stamp;
    StepPack* pack;            // the call's loss and range flag of this model, for one copy to the host (null: not asked)
    int nb1;                   // level-1 workgroups of this model
    int fcls, scls;            // entry j: the j-th model in forward-layout order / in update-form order (indices into the array)
    SortArgs so;               // entry c: the rank merge of the call's c-th grouping class
};
// launch 2.  Workgroups [0, ncls * mblk): class b / mblk's rank merge (mblk = 16 F); then the (model, tile) pairs, a model's tiles
// neighbours as in the solo step.  A model's tile 0 clears its owner count (sortB_body clears the class's: the first model's).
__device__ __forceinline__ void step_pick(const StepArg* __restrict__ args, const int ncls, const int mblk, const int first, const int tiles,
                                          int& m, int& tile)
{
    const int lin = (int)blockIdx.x - ncls * mblk;
    m = args[first + lin / tiles].fcls;
    tile = lin % tiles;
    if (tile == 0 && threadIdx.x == 0) *args[m].sa.owner_cnt = 0;
}
template <typename KT, int NF, bool WV>
__global__ __launch_bounds__(256) void k_fm_step_fwd(const StepArg* __restrict__ args, const int ncls, const int mblk, const int first,
                                                     const int tiles)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ float s_gb[16];
    if ((int)blockIdx.x < ncls * mblk) { const SortArgs so = args[(int)blockIdx.x / mblk].so; sortB_body<KT>(so, (int)blockIdx.x % mblk, smem); return; }
    int m, tile;
    step_pick(args, ncls, mblk, first, tiles, m, tile);
    const FmArgs a = args[m].a;
    fm_body<NF, WV>(a, tile, s_gb);
}
template <typename KT, int L, int NC, bool WV>
__global__ __launch_bounds__(256) void k_fm_step_fwd_wide(const StepArg* __restrict__ args, const int ncls, const int mblk, const int first,
                                                          const int tiles)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ float s_gb[256 / L];
    if ((int)blockIdx.x < ncls * mblk) { const SortArgs so = args[(int)blockIdx.x / mblk].so; sortB_body<KT>(so, (int)blockIdx.x % mblk, smem); return; }
    int m, tile;
    step_pick(args, ncls, mblk, first, tiles, m, tile);
    const FmArgs a = args[m].a;
    fm_wide_body<L, NC, WV>(a, tile, s_gb);
}
// the class's marks into the model's own array: a segment head whose row the rank merge (a launch earlier) marked
__device__ __forceinline__ void step_copy_marks(const StepArg& g, const ScatArgs& sa, const int blk, const int nblk)
{
    if (!g.own_marks) return;
    const int n = sa.F * sa.N2;
    for (int i = blk * 256 + (int)threadIdx.x; i < n; i += nblk * 256) {
        const int4 r = sa.rec[i];
        if (r.x >= 0 && (i % sa.N2) == r.z && sa.tag_shared[r.x] == sa.stamp) g.own_marks[r.x] = g.own_stamp;
    }
}
// launch 3: grid (nb1 of the largest model, models of the form)
template <bool SHARED>
__global__ __launch_bounds__(256) void k_fm_step_scat1(const StepArg* __restrict__ args, const int first)
{
    const int m = args[first + blockIdx.y].scls;
    const int nb1 = args[m].nb1;
    if ((int)blockIdx.x >= nb1) return;
    const ScatArgs sa = args[m].sa;
    if (SHARED) step_copy_marks(args[m], sa, blockIdx.x, nb1);
    scat1h_form<SHARED>(sa, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_fm_step_scatw1(const StepArg* __restrict__ args, const int first)
{
    const int m = args[first + blockIdx.y].scls;
    const int nb1 = args[m].nb1;
    if ((int)blockIdx.x >= nb1) return;
    const ScatArgs sa = args[m].sa;
    step_copy_marks(args[m], sa, blockIdx.x, nb1);
    scatw1_body(sa, blockIdx.x);
}
// launch 4: grid (1 + 256, models of the form).  The tail's workgroup also hands the model's loss and range flag to the call's
// packed array (the forwards that raise the flag ran two launches earlier) and clears a raised flag, as fm_sync does.
__device__ __forceinline__ void step_tail(const StepArg& g, float* sl)
{
    const StepTail t = g.t;
    fm_tail_body(t.b, t.gb_part, t.n, t.lr, t.lambda, t.loss_t, t.Ba, t.lscale, t.loss_out, sl, t.bo);
    if (threadIdx.x == 0 && g.pack) {
        const int flag = *static_cast<volatile int*>(g.a.err);
        g.pack->loss = *t.loss_out; g.pack->flag = flag;
        if (flag) *g.a.err = 0;
    }
}
template <bool SHARED>
__global__ __launch_bounds__(256) void k_fm_step_scat2_tail(const StepArg* __restrict__ args, const int first)
{
    __shared__ float s_l[256];
    const int m = args[first + blockIdx.y].scls;
    if (blockIdx.x == 0) { step_tail(args[m], s_l); return; }
    const ScatArgs sa = args[m].sa;
    scat2w_form<SHARED>(sa, (int)blockIdx.x - 1, (int)gridDim.x - 1);
}
__global__ __launch_bounds__(256) void k_fm_step_scatw2_tail(const StepArg* __restrict__ args, const int first)
{
    __shared__ double s_w[1024];
    const int m = args[first + blockIdx.y].scls;
    if (blockIdx.x == 0) { step_tail(args[m], reinterpret_cast<float*>(s_w)); return; }
    const ScatArgs sa = args[m].sa;
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

// (the argument arrays of the group calls reach the device through an ArgRing of the handle in front: arg_ring.h)

}  // namespace

struct fm_handle {
    std::string err; int dev = 0; hipStream_t st = nullptr; bool own_stream = false;
    int F = 0, K = 0, Bmax = 0, K1p = 0;
    bool wide = false;         // k >= 17: wide rows (fm_wide_body, scatw1_body / scatw2_body)
    int rw = SLOT;             // row stride in floats: SLOT for k <= 16, rup(k, 4) on the wide path
    int* noshare = nullptr;    // wide path: [n_rows] zeros, the scatter's tag_shared (every row takes the plain read-modify-write)
    float* table16 = nullptr; int64_t n_rows = 0; float* b = nullptr; double scale = 1.0;
    float *gxp = nullptr, *loss_t = nullptr, *gb_part = nullptr, *loss_dev = nullptr; int* err_flag = nullptr;
    RowGroupBufs rg; void* skeys = nullptr;     // the batch's grouping (sparse_rows.hip.h); skeys: phase-A output of the split sort
    double* cpow1 = nullptr; bool key64 = true;
    // Adam / FTRL (fm_set_optimizer): compact state s0 / s1 [n_rows, K], the bias's sb [2], gradient store G [n_rows, rw],
    // stamp [n_rows]; t = steps since the state was initialised.  dense_g: FM_OPT_DENSE_G=1, the A/B variant of k_fm_opt_pass.
    int opt = FM_OPT_SGD; float beta1 = 0.9f, beta2 = 0.999f, eps = 1e-8f; int64_t t = 0; bool dense_g = false;
    int scat_form = SCAT1_HALF;      // FNN_SCAT1_FORM (scat1_blocks)
    int scat2_form = SCAT2_WAVE;     // FNN_SCAT2_FORM: level 2 of the narrow rows (scat2w_body; block: scat2_body)
    int sort_merge4 = 0;       // FNN_SORT_RUNS=4|16 (sortA_body; default 16: the run sort is a launch of its own here)
    float *s0 = nullptr, *s1 = nullptr, *sb = nullptr, *G = nullptr; int* stamp = nullptr;
    // fm_set_shared_rows: tag_first / tag_shared [n_rows] of SortArgs, allocated with the table while the mode is on (kept when it
    // goes off); tag_stamp: the last grouping's stamp (25 bits, then both arrays start over); step_stamp: the stamp of the last
    // training step under the mode, 0 = none yet -- what fm_count_shared_rows scans for.
    bool shared = false; int* tag_first = nullptr; int* tag_shared = nullptr; int tag_stamp = 0, step_stamp = 0;
    unsigned long long* mark_cnt = nullptr;
    // fm_train_online: the examples one launch may take (FM_ONLINE_CHUNK, read at fm_create) and the call's loss accumulators
    int64_t online_chunk = 65536; fm_online::Out* online_out = nullptr;
    // The group calls, used when this handle is hs[0]: the argument rings of fm_train_online_multi (eight launches of the largest
    // group, 1 MiB), fm_train_step_multi and fm_predict_multi / fm_eval_multi (four calls of the largest group each); the event
    // that joins the other members' streams to this one's and back (GroupCall); the packed {loss, range flag} of an
    // fm_train_step_multi call that asks for the losses
    ArgRing online_ring{sizeof(fm_online::Args), 8 * FM_ONLINE_MAX_MODELS};
    ArgRing step_ring{sizeof(StepArg), 4 * FM_STEP_MAX_MODELS};
    ArgRing eval_ring{sizeof(EvalArg), 4 * FM_EVAL_MAX_MODELS};
    hipEvent_t join = nullptr; StepPack* step_pack = nullptr;
};

#define MHK(h, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_); return FNN_ERR_HIP; } } while (0)
#define MFAIL(h, code, msg) do { (h)->err = (msg); return (code); } while (0)

namespace {

int fold_scale(fm_handle* h)          // fold the lazy decay back into the rows
{
    if (h->scale == 1.0 || !h->table16) return FNN_OK;
    const size_t n = (size_t)h->n_rows * h->rw;
    hipLaunchKernelGGL(k_fm_rescale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->table16, n, (float)h->scale);
    MHK(h, hipGetLastError());
    h->scale = 1.0;
    return FNN_OK;
}

// (Re)allocate and zero the shared-row tags for the current table; the stamps start over.
int alloc_tags(fm_handle* h)
{
    for (int** p : {&h->tag_first, &h->tag_shared}) { if (*p) hipFree(*p); *p = nullptr; }
    h->tag_stamp = h->step_stamp = 0;
    if (!h->shared || !h->table16) return FNN_OK;
    for (int** p : {&h->tag_first, &h->tag_shared}) {
        MHK(h, hipMalloc((void**)p, (size_t)h->n_rows * sizeof(int)));
        MHK(h, hipMemsetAsync(*p, 0, (size_t)h->n_rows * sizeof(int), h->st));
    }
    MHK(h, hipStreamSynchronize(h->st));
    return FNN_OK;
}
// a fresh stamp for the grouping of the step about to run (next_stamp of fnn_api.hip): 2^25 groupings, then the tags start over
int fm_next_stamp(fm_handle* h)
{
    if (h->tag_stamp >= (1 << 25) - 1) {
        hipMemsetAsync(h->tag_first, 0, (size_t)h->n_rows * sizeof(int), h->st);
        hipMemsetAsync(h->tag_shared, 0, (size_t)h->n_rows * sizeof(int), h->st);
        h->tag_stamp = 0;
    }
    h->step_stamp = ++h->tag_stamp;
    return h->step_stamp;
}
// the claim of the rank merge (sortB_body): on only while the mode is
void set_claim(fm_handle* h, SortArgs& so)
{
    if (!h->shared) return;
    so.tag_first = h->tag_first; so.tag_shared = h->tag_shared; so.stamp = fm_next_stamp(h);
}

size_t opt_state_len(const fm_handle* h) { return ((size_t)h->n_rows * h->K + 3) & ~(size_t)3; }

// Free and, under Adam / FTRL, allocate and initialise the optimiser state for the current table; resets the step count.
int init_opt_state(fm_handle* h)
{
    for (float** p : {&h->s0, &h->s1, &h->G}) { if (*p) hipFree(*p); *p = nullptr; }
    if (h->stamp) hipFree(h->stamp);
    h->stamp = nullptr; h->t = 0;
    if (h->opt == FM_OPT_SGD) return FNN_OK;
    const float sb[2] = {h->opt == FM_OPT_FTRL ? 0.1f : 0.f, 0.f};
    MHK(h, hipMemcpy(h->sb, sb, 8, hipMemcpyHostToDevice));
    if (!h->table16) return FNN_OK;
    const size_t n = opt_state_len(h);
    MHK(h, hipMalloc((void**)&h->s0, n * 4)); MHK(h, hipMalloc((void**)&h->s1, n * 4));
    MHK(h, hipMalloc((void**)&h->G, (size_t)h->n_rows * h->rw * 4)); MHK(h, hipMalloc((void**)&h->stamp, (size_t)h->n_rows * 4));
    MHK(h, hipMemsetAsync(h->s1, 0, n * 4, h->st)); MHK(h, hipMemsetAsync(h->G, 0, (size_t)h->n_rows * h->rw * 4, h->st));
    MHK(h, hipMemsetAsync(h->stamp, 0, (size_t)h->n_rows * 4, h->st));
    if (h->opt == FM_OPT_FTRL) hipLaunchKernelGGL(k_fm_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->s0, n, 0.1f);
    else MHK(h, hipMemsetAsync(h->s0, 0, n * 4, h->st));
    MHK(h, hipGetLastError());
    MHK(h, hipStreamSynchronize(h->st));
    return FNN_OK;
}

// The forwards of both layouts, one instantiation per 16 fields: NF = NC = ceil(F / 16) (1 up to 16 fields).  sb: the rank merge
// of the batch's sort runs beside the forward (training), null: the forward alone (predictions).  nb: the examples' workgroups.
// WV = (a.wts != nullptr): without weights the kernels are the ones that never read a weight.
template <typename KT, int N, bool WV>
void launch_fwd_nw(const fm_handle* h, const SortArgs* sb, const FmArgs& a, int nb)
{
    if (!h->wide) {
        if (!sb) hipLaunchKernelGGL((k_fm<N, WV>), dim3(nb), dim3(256), 0, h->st, a);
        else hipLaunchKernelGGL((k_fm_merge_fwd<KT, N, WV>), dim3(sb->nblk + nb), dim3(256), sort_lds_bytes<KT>(), h->st, *sb, a);
    } else if (h->rw <= 64) {         // L = 16 lanes per example while a row's float4 pieces fit (rank <= 63), else 32
        if (!sb) hipLaunchKernelGGL((k_fm_wide<16, N, WV>), dim3(nb), dim3(256), 0, h->st, a);
        else hipLaunchKernelGGL((k_fm_wide_merge_fwd<KT, 16, N, WV>), dim3(sb->nblk + nb), dim3(256), sort_lds_bytes<KT>(), h->st, *sb, a);
    } else {
        if (!sb) hipLaunchKernelGGL((k_fm_wide<32, N, WV>), dim3(nb), dim3(256), 0, h->st, a);
        else hipLaunchKernelGGL((k_fm_wide_merge_fwd<KT, 32, N, WV>), dim3(sb->nblk + nb), dim3(256), sort_lds_bytes<KT>(), h->st, *sb, a);
    }
}
template <typename KT, int N>
void launch_fwd_n(const fm_handle* h, const SortArgs* sb, const FmArgs& a, int nb)
{
    if (a.wts) launch_fwd_nw<KT, N, true>(h, sb, a, nb);
    else launch_fwd_nw<KT, N, false>(h, sb, a, nb);
}
template <typename KT>
void launch_fwd(const fm_handle* h, const SortArgs* sb, const FmArgs& a, int nb)
{
    switch ((h->F + 15) / 16) {
    case 1: launch_fwd_n<KT, 1>(h, sb, a, nb); break;
    case 2: launch_fwd_n<KT, 2>(h, sb, a, nb); break;
    case 3: launch_fwd_n<KT, 3>(h, sb, a, nb); break;
    default: launch_fwd_n<KT, 4>(h, sb, a, nb); break;
    }
}
// The forwards of a group of models (eval_forward): cls 0 narrow rows, 1 wide at 16 lanes an example, 2 wide at 32.
template <int N, bool WV>
void launch_multi_nw(hipStream_t st, int cls, dim3 grid, const EvalArg* args, int first, int nm, int64_t tiles, int model_fast)
{
    if (cls == 0) hipLaunchKernelGGL((k_fm_multi<N, WV>), grid, dim3(256), 0, st, args, first, nm, tiles, model_fast);
    else if (cls == 1) hipLaunchKernelGGL((k_fm_wide_multi<16, N, WV>), grid, dim3(256), 0, st, args, first, nm, tiles, model_fast);
    else hipLaunchKernelGGL((k_fm_wide_multi<32, N, WV>), grid, dim3(256), 0, st, args, first, nm, tiles, model_fast);
}
template <int N>
void launch_multi_n(bool wv, hipStream_t st, int cls, dim3 grid, const EvalArg* args, int first, int nm, int64_t tiles, int model_fast)
{
    if (wv) launch_multi_nw<N, true>(st, cls, grid, args, first, nm, tiles, model_fast);
    else launch_multi_nw<N, false>(st, cls, grid, args, first, nm, tiles, model_fast);
}

// The wide path's forward: 256 / L examples per workgroup (L = 16 while rank <= 63, else 32).
int wide_epb(const fm_handle* h) { return h->rw <= 64 ? 16 : 8; }

// Adam's / FTRL's pass over the table (k_fm_opt_pass).  Defined below fm_step: the kernel templates are instantiated in the order
// of their first use, and that order is the order of the functions in the device code.
void launch_opt_pass(fm_handle* h, float lambda, float lr_step);

// fm_train_step_multi: launch 2 of a layout: lay 0 narrow rows, 1 wide at 16 lanes an example, 2 wide at 32; ncls > 0: the classes' rank merges in front
template <typename KT, int N, bool WV>
void launch_step_fwd_nw(hipStream_t st, int lay, const StepArg* d, int ncls, int mblk, int first, int nm, int tiles)
{
    const dim3 grid((unsigned)(ncls * mblk + nm * tiles));
    const size_t lds = ncls ? sort_lds_bytes<KT>() : 0;
    if (lay == 0) hipLaunchKernelGGL((k_fm_step_fwd<KT, N, WV>), grid, dim3(256), lds, st, d, ncls, mblk, first, tiles);
    else if (lay == 1) hipLaunchKernelGGL((k_fm_step_fwd_wide<KT, 16, N, WV>), grid, dim3(256), lds, st, d, ncls, mblk, first, tiles);
    else hipLaunchKernelGGL((k_fm_step_fwd_wide<KT, 32, N, WV>), grid, dim3(256), lds, st, d, ncls, mblk, first, tiles);
}
template <typename KT>
void launch_step_fwd(hipStream_t st, int F, bool wv, int lay, const StepArg* d, int ncls, int mblk, int first, int nm, int tiles)
{
#define FM_STEP_FWD(N) do { if (wv) launch_step_fwd_nw<KT, N, true>(st, lay, d, ncls, mblk, first, nm, tiles); \
                            else launch_step_fwd_nw<KT, N, false>(st, lay, d, ncls, mblk, first, nm, tiles); } while (0)
    switch ((F + 15) / 16) {
    case 1: FM_STEP_FWD(1); break;
    case 2: FM_STEP_FWD(2); break;
    case 3: FM_STEP_FWD(3); break;
    default: FM_STEP_FWD(4); break;
    }
#undef FM_STEP_FWD
}

bool fm_wt_env() { return !(getenv("FM_WT") && atoi(getenv("FM_WT")) == 0); }     // gx' written through unless FM_WT=0

// The forward's arguments of a prediction (fm_predict_w, fm_eval_w; B = N: a member of fm_predict_multi / fm_eval_multi)
FmArgs predict_args(const fm_handle* h, const int32_t* ids, const float* wts, int B, float* p_out, bool wt)
{
    return FmArgs{ids, nullptr, B, h->F, h->K, h->table16, h->n_rows, h->b, (float)h->scale, 1.0f, 0, h->gxp, h->K1p, p_out,
                  h->loss_t, h->gb_part, h->err_flag, wt, nullptr, (int)h->t, h->rw, wts};
}

int fm_forward(fm_handle* h, const int32_t* ids, const float* wts, int B, float* p_out)
{
    const int ex = h->wide ? wide_epb(h) : 16;
    launch_fwd<unsigned>(h, nullptr, predict_args(h, ids, wts, B, p_out, fm_wt_env()), rup(B, ex) / ex);
    MHK(h, hipGetLastError());
    return FNN_OK;
}

// One optimiser step of one handle, as arguments: the forward + gradients (a; p.t.n workgroups of examples), both levels of the
// sparse-row update (sa; nb1 workgroups at level 1) and the bias / loss tail (t); lr_step: Adam's bias-corrected step size, else
// lr.  The solo step (fm_step) launches its kernels with these; fm_train_step_multi stores them in the model's StepArg.
//   lead, stamp  the handle whose grouping (rec, shared-row marks) the update reads, and that grouping's stamp: h itself and the
//                stamp it just claimed in a solo step, the grouping class's first model in a group
//   form1, form2 levels 1 / 2 of the narrow rows: the handle's own choice in a solo step without shared rows, else SCAT1_HALF /
//                SCAT2_WAVE (shared rows have no other form; every form gives the same bits)
// The step's changes to the handle happen here, in this order: the step count (Adam / FTRL), a.scale, then SGD's dense L2
// decay as the lazy scale, then the update's lr / scale: touched rows get stored -= lr * g / scale.  Adam / FTRL: the same
// sorted sums land in the zeroed gradient store, G[row] = G[row] - (-1) * sum.
struct StepPlan { FmArgs a; ScatArgs sa; StepTail t; int nb1; float lr_step; };
StepPlan plan_step(fm_handle* h, const int32_t* ids, const float* wts, const float* y, int B, float lr, float lambda, int reduce_mean,
                   float* p_out, bool wt, const fm_handle* lead, int stamp, int form1, int form2)
{
    StepPlan p;
    const int F = h->F, ex = h->wide ? wide_epb(h) : 16, Ba = rup(B, ex);
    const bool opt = h->opt != FM_OPT_SGD;
    const float dscale = reduce_mean ? 1.0f / (float)B : 1.0f;
    p.lr_step = lr;
    if (opt) {
        h->t += 1;
        if (h->opt == FM_OPT_ADAM)                 // TensorFlow's bias-corrected step size lr_t
            p.lr_step = (float)((double)lr * std::sqrt(1.0 - std::pow((double)h->beta2, (double)h->t)) /
                                (1.0 - std::pow((double)h->beta1, (double)h->t)));
    }
    p.a = FmArgs{ids, y, B, F, h->K, h->table16, h->n_rows, h->b, (float)h->scale, dscale, 1, h->gxp, h->K1p, p_out, h->loss_t,
                 h->gb_part, h->err_flag, wt, opt && !h->dense_g ? h->stamp : nullptr, (int)h->t, h->rw, wts};
    if (!opt) h->scale *= 1.0 - (double)lr * (double)lambda;
    RowGroupBufs rg = h->rg;
    rg.rec = lead->rg.rec;
    p.sa = scat_args(rg, SORT_N, F, h->K, h->gxp, h->K1p, h->cpow1, opt ? -1.0 : (double)lr / h->scale, opt ? h->G : h->table16, h->rw);
    if (h->shared) { p.sa.tag_shared = lead->tag_shared; p.sa.stamp = stamp; }
    else if (h->wide) { p.sa.tag_shared = h->noshare; p.sa.stamp = 1; }
    if (h->wide) {
        p.sa.gxf = h->rw;
        p.nb1 = (F * (SORT_N / WCH) * (h->rw / 4) + 255) / 256;
    } else {
        p.nb1 = scat1_blocks(p.sa, form1);         // also chooses sa.form
        p.sa.form2 = form2;
    }
    p.t = StepTail{h->b, h->gb_part, Ba / ex, lr, lambda, h->loss_t, Ba, dscale, h->loss_dev,
                   opt ? FmBiasOpt{h->opt, h->sb, p.lr_step, h->beta1, h->beta2, h->eps} : FmBiasOpt{FM_OPT_SGD, nullptr, 0.f, 0.f, 0.f, 0.f}};
    return p;
}

// The solo step, narrow and wide rows: the run sort; the forward + gradients beside the rank merge; level 1 of the sparse-row
// update; level 2 beside the bias / loss tail; then Adam's / FTRL's pass over the table, or the fold of SGD's lazy scale where due.
int fm_step(fm_handle* h, const int32_t* ids, const float* wts, const float* y, int B, float lr, float lambda, int reduce_mean, float* p_out)
{
    const int F = h->F;
    SortArgs so{ids, B, F, h->n_rows, h->rg.rec, h->rg.owner_cnt, 4 * F, h->skeys};
    so.merge4 = h->sort_merge4;
    SortArgs sb = so; sb.nblk = 16 * F;
    set_claim(h, sb);
    const bool own_forms = !h->wide && !h->shared;
    const StepPlan p = plan_step(h, ids, wts, y, B, lr, lambda, reduce_mean, p_out, fm_wt_env(), h, sb.stamp,
                                 own_forms ? h->scat_form : SCAT1_HALF, own_forms ? h->scat2_form : SCAT2_WAVE);
    const StepTail& t = p.t;
    launch_sort_runs(h->st, h->key64, so);
    if (h->key64) launch_fwd<unsigned long long>(h, &sb, p.a, t.n);
    else launch_fwd<unsigned>(h, &sb, p.a, t.n);
#define FM_SCAT(k1, k2_tail) do { \
        hipLaunchKernelGGL(k1, dim3(p.nb1), dim3(256), 0, h->st, p.sa); \
        hipLaunchKernelGGL(k2_tail, dim3(1 + 256), dim3(256), 0, h->st, p.sa, t.b, t.gb_part, t.n, t.lr, t.lambda, t.loss_t, t.Ba, t.lscale, \
                           t.loss_out, t.bo); } while (0)
    if (h->wide) FM_SCAT(k_fm_scatw1, k_fm_scatw2_tail);
    else if (h->shared) FM_SCAT(k_fm_scat1s, k_fm_scat2s_tail);          // the SHARED forms, with the marks of this step's rank merge
    else FM_SCAT(k_scat1, k_fm_scat2_tail);
#undef FM_SCAT
    MHK(h, hipGetLastError());
    if (h->opt != FM_OPT_SGD) { launch_opt_pass(h, lambda, p.lr_step); MHK(h, hipGetLastError()); return FNN_OK; }
    if (h->scale < 5.96e-8 || h->scale > 1.0) return fold_scale(h);
    return FNN_OK;
}

void launch_opt_pass(fm_handle* h, float lambda, float lr_step)
{
    const size_t nk = (size_t)h->n_rows * h->K;
    const dim3 grid((unsigned)(((nk + 3) / 4 + 255) / 256));
    if (h->dense_g)
        hipLaunchKernelGGL(k_fm_opt_pass<true>, grid, dim3(256), 0, h->st, h->table16, h->G, h->stamp, (int)h->t, h->s0, h->s1, nk, h->K,
                           h->rw, lambda, h->opt, lr_step, h->beta1, h->beta2, h->eps);
    else
        hipLaunchKernelGGL(k_fm_opt_pass<false>, grid, dim3(256), 0, h->st, h->table16, h->G, h->stamp, (int)h->t, h->s0, h->s1, nk, h->K,
                           h->rw, lambda, h->opt, lr_step, h->beta1, h->beta2, h->eps);
}

// ArgRing (arg_ring.h) with the failure's text left on the handle in front
int ring_take(fm_handle* h0, ArgRing& r, size_t n, size_t* slot)
{
    MHK(h0, fnn::ring_take(r, n, slot));
    return FNN_OK;
}
int ring_send(fm_handle* h0, ArgRing& r, size_t slot, size_t n)
{
    MHK(h0, fnn::ring_send(r, slot, n, h0->st));
    return FNN_OK;
}

// A call on a list of fm handles: GroupCall (group_call.h), refusals without a usable hs[0] left with fm_last_error(NULL).
// fold_scale(), fm_next_stamp() and launch_opt_pass() work on their handle's stream: on_stream() gives them hs[0]'s.
using FmGroup = GroupCall<fm_handle>;
int check_tables(const FmGroup& g)
{
    for (int m = 0; m < g.n; ++m) if (!g.hs[m]->table16) return g.refuse(FNN_ERR_STATE, g.at("fm_set_table has not been called", m));
    return FNN_OK;
}

}  // namespace

extern "C" {

const char* fm_last_error(const fm_handle* h) { return h ? h->err.c_str() : g_fm_err.c_str(); }

int fm_create(int n_fields, int k, int max_batch, int device, void* stream, fm_handle** out)
{
    if (!out) { g_fm_err = "null argument"; return FNN_ERR_ARG; }
    *out = nullptr;
    if (n_fields < 1 || n_fields > 64 || k < 1 || k > 128 || max_batch < 1 || max_batch > SORT_N) {
        g_fm_err = "need 1 <= n_fields <= 64, 1 <= k <= 128 (rank 0..127), 1 <= max_batch <= 4096"; return FNN_ERR_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_fm_err = "no HIP device (libfnn_hip.so has no CPU fallback)"; return FNN_ERR_HIP; }
    fm_handle* h = new fm_handle();
    h->dev = device; h->F = n_fields; h->K = k; h->Bmax = max_batch;
    h->wide = k > 16; h->rw = h->wide ? rup(k, 4) : SLOT;
    h->K1p = h->wide ? n_fields * h->rw : rup(n_fields, 16) * SLOT;   // gx' of an example: a slot per field of rup(F, 16), or [F][rw]
    auto fail = [&](int code) { g_fm_err = h->err; fm_destroy(h); return code; };
#define FK(expr) do { hipError_t e2_ = (expr); if (e2_ != hipSuccess) { h->err = std::string(#expr) + ": " + hipGetErrorString(e2_); return fail(FNN_ERR_HIP); } } while (0)
    FK(hipSetDevice(h->dev));
    if (stream) h->st = (hipStream_t)stream; else { FK(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking)); h->own_stream = true; }
    auto al = [&](void** p, size_t bytes) { hipError_t e = hipMalloc(p, bytes); if (e == hipSuccess) e = hipMemsetAsync(*p, 0, bytes, h->st); return e; };
    const size_t Ba = rup(h->Bmax, 16);
    FK(al((void**)&h->gxp, Ba * h->K1p * 4)); FK(al((void**)&h->loss_t, Ba * 4)); FK(al((void**)&h->gb_part, (Ba / 8) * 4));
    FK(al((void**)&h->loss_dev, 4)); FK(al((void**)&h->b, 4)); FK(al((void**)&h->err_flag, 4)); FK(al((void**)&h->sb, 8));
    FK(al((void**)&h->mark_cnt, 8)); FK(al((void**)&h->online_out, sizeof(fm_online::Out)));
    FK(row_group_alloc(h->rg, h->F, SORT_N, h->wide, h->rw, h->st, /*owners16*/ true));
    FK(al(&h->skeys, (size_t)h->F * SORT_N * 8));
    {
        std::vector<double> ones(SORT_N + 1, 1.0);                   // no per-touch decay: every power is 1
        FK(hipMalloc((void**)&h->cpow1, ones.size() * 8));
        FK(hipMemcpy(h->cpow1, ones.data(), ones.size() * 8, hipMemcpyHostToDevice));
    }
    FK(hipStreamSynchronize(h->st));
#undef FK
    h->dense_g = getenv("FM_OPT_DENSE_G") && atoi(getenv("FM_OPT_DENSE_G")) == 1;
    h->scat_form = scat1_form_env();
    h->scat2_form = scat2_form_env();
    h->sort_merge4 = sort_merge4_env(0);
    if (const char* e = getenv("FM_ONLINE_CHUNK")) { const long long c = atoll(e); if (c >= 1) h->online_chunk = c; }
    *out = h;
    return FNN_OK;
}

int fm_destroy(fm_handle* h)
{
    if (!h) return FNN_ERR_ARG;
    hipSetDevice(h->dev);
    if (h->st) hipStreamSynchronize(h->st);
    void* ptrs[] = {h->table16, h->b, h->gxp, h->loss_t, h->gb_part, h->loss_dev, h->err_flag, h->skeys, h->cpow1, h->s0, h->s1,
                    h->sb, h->G, h->stamp, h->noshare, h->tag_first, h->tag_shared, h->mark_cnt, h->online_out, h->step_pack};
    for (void* p : ptrs) if (p) hipFree(p);
    for (ArgRing* r : {&h->online_ring, &h->step_ring, &h->eval_ring}) ring_release(*r);
    if (h->join) hipEventDestroy(h->join);
    row_group_free(h->rg);
    if (h->own_stream && h->st) hipStreamDestroy(h->st);
    delete h;
    return FNN_OK;
}

int fm_sync(fm_handle* h)
{
    if (!h) return FNN_ERR_ARG;
    int flag = 0;
    MHK(h, hipMemcpyAsync(&flag, h->err_flag, 4, hipMemcpyDeviceToHost, h->st));
    MHK(h, hipStreamSynchronize(h->st));
    if (flag) { MHK(h, hipMemsetAsync(h->err_flag, 0, 4, h->st)); MFAIL(h, FNN_ERR_RANGE, "feature id outside [-1, n_rows)"); }
    return FNN_OK;
}

int fm_set_table(fm_handle* h, const float* rows, int64_t n_rows)
{
    if (!h || !rows || n_rows < 1 || n_rows >= (1ll << 31)) return FNN_ERR_ARG;
    MHK(h, hipSetDevice(h->dev));
    MHK(h, hipStreamSynchronize(h->st));
    if (h->table16) { hipFree(h->table16); h->table16 = nullptr; }
    if (h->noshare) { hipFree(h->noshare); h->noshare = nullptr; }
    MHK(h, hipMalloc((void**)&h->table16, (size_t)n_rows * h->rw * 4));
    if (h->wide) {
        MHK(h, hipMalloc((void**)&h->noshare, (size_t)n_rows * 4));
        MHK(h, hipMemsetAsync(h->noshare, 0, (size_t)n_rows * 4, h->st));
    }
    float* tmp = nullptr;
    MHK(h, hipMalloc((void**)&tmp, (size_t)n_rows * h->K * 4));
    MHK(h, hipMemcpy(tmp, rows, (size_t)n_rows * h->K * 4, hipMemcpyHostToDevice));
    const size_t n = (size_t)n_rows * h->rw;
    hipLaunchKernelGGL(k_pack_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, tmp, n_rows, h->K, h->rw, h->table16);
    MHK(h, hipStreamSynchronize(h->st));
    hipFree(tmp);
    h->n_rows = n_rows; h->scale = 1.0;
    h->key64 = (unsigned long long)n_rows * SORT_N > 0xFFFFFFFFull;
    const int rct = alloc_tags(h);                                // the tags are sized by the table
    if (rct != FNN_OK) return rct;
    return init_opt_state(h);                                     // fresh state for the new rows
}

static int fm_rows(fm_handle* h, const int64_t* row_ids, int64_t n, float* out)
{
    if (!h->table16) MFAIL(h, FNN_ERR_STATE, "fm_set_table has not been called");
    MHK(h, hipSetDevice(h->dev));
    int rc = fold_scale(h);
    if (rc != FNN_OK) return rc;
    int64_t* di = nullptr; float* dout = nullptr;
    if (row_ids) { MHK(h, hipMalloc((void**)&di, n * 8)); MHK(h, hipMemcpy(di, row_ids, n * 8, hipMemcpyHostToDevice)); }
    MHK(h, hipMalloc((void**)&dout, (size_t)n * h->K * 4));
    const size_t cnt = (size_t)n * h->K;
    hipLaunchKernelGGL(k_unpack_rows, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->st, h->table16, di, n, h->n_rows, h->K, h->rw,
                       dout, h->err_flag);
    MHK(h, hipMemcpyAsync(out, dout, cnt * 4, hipMemcpyDeviceToHost, h->st));
    rc = fm_sync(h);
    if (di) hipFree(di);
    hipFree(dout);
    return rc;
}

int fm_get_table(fm_handle* h, float* rows_out) { if (!h || !rows_out) return FNN_ERR_ARG; return fm_rows(h, nullptr, h->n_rows, rows_out); }
int fm_get_rows(fm_handle* h, const int64_t* row_ids, int64_t n, float* out)
{
    if (!h || !row_ids || !out || n < 1) return FNN_ERR_ARG;
    return fm_rows(h, row_ids, n, out);
}

int fm_set_b(fm_handle* h, float b)
{
    if (!h) return FNN_ERR_ARG;
    MHK(h, hipSetDevice(h->dev)); MHK(h, hipStreamSynchronize(h->st));
    MHK(h, hipMemcpy(h->b, &b, 4, hipMemcpyHostToDevice));
    return FNN_OK;
}
int fm_get_b(fm_handle* h, float* b)
{
    if (!h || !b) return FNN_ERR_ARG;
    MHK(h, hipSetDevice(h->dev)); MHK(h, hipStreamSynchronize(h->st));
    MHK(h, hipMemcpy(b, h->b, 4, hipMemcpyDeviceToHost));
    return FNN_OK;
}

int fm_train_step(fm_handle* h, const int32_t* ids, const float* y, int B, float lr, float lambda, int reduce_mean, float* p_out,
                  float* loss_out)
{
    return fm_train_step_w(h, ids, nullptr, y, B, lr, lambda, reduce_mean, p_out, loss_out);
}

int fm_train_step_w(fm_handle* h, const int32_t* ids, const float* wts, const float* y, int B, float lr, float lambda, int reduce_mean,
                    float* p_out, float* loss_out)
{
    if (!h || !ids || !y) return FNN_ERR_ARG;
    if (B < 1 || B > h->Bmax) MFAIL(h, FNN_ERR_ARG, "B must be in [1, max_batch]");
    if (!h->table16) MFAIL(h, FNN_ERR_STATE, "fm_set_table has not been called");
    if (h->opt == FM_OPT_SGD && (!(lr * lambda < 1.0f) || lambda < 0.f)) MFAIL(h, FNN_ERR_ARG, "need 0 <= lr * lambda < 1");
    if (h->opt != FM_OPT_SGD && (!(lambda >= 0.f) || !(lr > 0.f))) MFAIL(h, FNN_ERR_ARG, "Adam / FTRL need lr > 0 and lambda >= 0");
    MHK(h, hipSetDevice(h->dev));
    int rc = fm_step(h, ids, wts, y, B, lr, lambda, reduce_mean, p_out);
    if (rc != FNN_OK) return rc;
    if (loss_out) {
        MHK(h, hipMemcpyAsync(loss_out, h->loss_dev, 4, hipMemcpyDeviceToHost, h->st));
        return fm_sync(h);
    }
    return FNN_OK;
}

// The online schedule (fm_online.hip.h): one launch per run of examples, cut at FM_ONLINE_CHUNK and after the example whose decay
// takes the lazy scale out of [2^-24, 1] (fm_step's rule, so that online calls and batch steps fold at the same places).  A cut at
// the cap hands b (f32), the scale and the loss sum (f64) to the next launch unchanged: where it falls changes no bit.
int fm_train_online(fm_handle* h, const int32_t* ids, const float* wts, const float* y, int64_t N, float lr, float lambda, float* p_out,
                    double* loss_sum_out, float* loss_last_out)
{
    if (!h) return FNN_ERR_ARG;
    if (N < 0 || (N > 0 && (!ids || !y))) MFAIL(h, FNN_ERR_ARG, "need N >= 0, ids and y");
    if (h->opt != FM_OPT_SGD) MFAIL(h, FNN_ERR_STATE, "fm_train_online is plain SGD only (Adam / FTRL pass over the whole table per step)");
    if (!h->table16) MFAIL(h, FNN_ERR_STATE, "fm_set_table has not been called");
    if (!(lr * lambda < 1.0f) || lambda < 0.f) MFAIL(h, FNN_ERR_ARG, "need 0 <= lr * lambda < 1");
    if (loss_sum_out) *loss_sum_out = 0.0;
    if (loss_last_out) *loss_last_out = 0.f;
    if (N == 0) return FNN_OK;
    MHK(h, hipSetDevice(h->dev));
    MHK(h, hipMemsetAsync(h->online_out, 0, sizeof(fm_online::Out), h->st));
    const double dec = 1.0 - (double)lr * (double)lambda;
    for (int64_t n0 = 0; n0 < N;) {
        int64_t cnt = 0;
        double s = h->scale;
        bool fold = false;
        while (n0 + cnt < N && cnt < h->online_chunk && !fold) { s *= dec; ++cnt; fold = s < 5.96e-8 || s > 1.0; }
        const fm_online::Args a{ids + n0 * h->F, wts ? wts + n0 * h->F : nullptr, y + n0, cnt, h->F, h->K, h->rw, h->table16, h->n_rows, h->b,
                                h->scale, dec, lr, lambda, p_out ? p_out + n0 : nullptr, h->err_flag, h->online_out};
        hipLaunchKernelGGL(fm_online::k_fm_online, dim3(1), dim3(256), 0, h->st, a);
        MHK(h, hipGetLastError());
        h->scale = s;
        if (fold) { const int rc = fold_scale(h); if (rc != FNN_OK) return rc; }
        n0 += cnt;
    }
    if (loss_sum_out || loss_last_out) {
        fm_online::Out o{0.0, 0.f, 0.f};
        MHK(h, hipMemcpyAsync(&o, h->online_out, sizeof(o), hipMemcpyDeviceToHost, h->st));
        const int rc = fm_sync(h);
        if (loss_sum_out) *loss_sum_out = o.loss_sum;
        if (loss_last_out) *loss_last_out = o.loss_last;
        return rc;
    }
    return FNN_OK;
}

// Several models, one feed (fm_online::k_fm_online_multi), as a GroupCall: every launch on hs[0]'s stream, the argument array
// of each launch through hs[0]'s online_ring.
int fm_train_online_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const float* y, int64_t N,
                          const float* lr, const float* lambda, float* const* p_out, double* loss_sum_out, float* loss_last_out)
{
    FmGroup g("fm_train_online_multi", hs, n_models, FM_ONLINE_MAX_MODELS, g_fm_err);
    if (!hs || !lr || !lambda) return g.refuse(FNN_ERR_ARG, "null hs, lr or lambda");
    int rc = g.check_list("two workgroups would race on one table");
    if (rc != FNN_OK) return rc;
    if (N < 0 || (N > 0 && (!ids || !y))) return g.refuse(FNN_ERR_ARG, "need N >= 0, ids and y");
    for (int m = 0; m < n_models; ++m) {
        const float ll = lr[m] * lambda[m];
        if (!(ll >= 0.f && ll < 1.0f) || lambda[m] < 0.f) return g.refuse(FNN_ERR_ARG, g.at("need 0 <= lr * lambda < 1", m));
    }
    for (int m = 0; m < n_models; ++m)
        if (hs[m]->opt != FM_OPT_SGD) return g.refuse(FNN_ERR_STATE, g.at("plain SGD only (Adam / FTRL pass over the whole table per step)", m));
    rc = check_tables(g);
    if (rc != FNN_OK) return rc;
    for (int m = 0; m < n_models; ++m) {
        if (loss_sum_out) loss_sum_out[m] = 0.0;
        if (loss_last_out) loss_last_out[m] = 0.f;
    }
    if (N == 0) return FNN_OK;
    fm_handle* h0 = g.h0;
    rc = g.enter();
    if (rc != FNN_OK) return rc;
    const hipStream_t st = h0->st;
    int64_t chunk = h0->online_chunk;
    std::vector<double> dec(n_models), s(n_models);
    for (int m = 0; m < n_models; ++m) {
        MHK(h0, hipMemsetAsync(hs[m]->online_out, 0, sizeof(fm_online::Out), st));
        dec[m] = 1.0 - (double)lr[m] * (double)lambda[m];
        if (hs[m]->online_chunk < chunk) chunk = hs[m]->online_chunk;
    }
    for (int64_t n0 = 0; n0 < N;) {
        size_t slot = 0;
        rc = ring_take(h0, h0->online_ring, (size_t)n_models, &slot);
        if (rc != FNN_OK) return rc;
        // the launch ends after the first example whose decay takes ANY model's scale out of [2^-24, 1]
        int64_t cnt = 0;
        bool fold = false;
        for (int m = 0; m < n_models; ++m) s[m] = hs[m]->scale;
        while (n0 + cnt < N && cnt < chunk && !fold) {
            for (int m = 0; m < n_models; ++m) { s[m] *= dec[m]; fold = fold || s[m] < 5.96e-8 || s[m] > 1.0; }
            ++cnt;
        }
        fm_online::Args* a = h0->online_ring.at_host<fm_online::Args>(slot);
        for (int m = 0; m < n_models; ++m) {
            fm_handle* h = hs[m];
            a[m] = fm_online::Args{ids + n0 * h->F, wts ? wts + n0 * h->F : nullptr, y + n0, cnt, h->F, h->K, h->rw, h->table16, h->n_rows, h->b,
                                   h->scale, dec[m], lr[m], lambda[m], p_out && p_out[m] ? p_out[m] + n0 : nullptr, h->err_flag,
                                   h->online_out};
        }
        rc = ring_send(h0, h0->online_ring, slot, (size_t)n_models);
        if (rc != FNN_OK) return rc;
        hipLaunchKernelGGL(fm_online::k_fm_online_multi, dim3((unsigned)n_models), dim3(256), 0, st, h0->online_ring.at_dev<fm_online::Args>(slot));
        MHK(h0, hipGetLastError());
        for (int m = 0; m < n_models; ++m) {
            fm_handle* h = hs[m];
            h->scale = s[m];
            if (s[m] < 5.96e-8 || s[m] > 1.0) {
                const int rf = on_stream(h, st, [&] { return fold_scale(h); });
                if (rf != FNN_OK) return g.member_failed(rf, h, m);
            }
        }
        n0 += cnt;
    }
    rc = g.leave();
    if (rc != FNN_OK || (!loss_sum_out && !loss_last_out)) return rc;
    std::string bad;
    for (int m = 0; m < n_models; ++m) {
        fm_handle* h = hs[m];
        fm_online::Out o{0.0, 0.f, 0.f};
        MHK(h0, hipMemcpyAsync(&o, h->online_out, sizeof(o), hipMemcpyDeviceToHost, h->st));
        const int rm = fm_sync(h);
        if (rm == FNN_ERR_RANGE) eval_list_add(bad, m);
        else if (rm != FNN_OK) return g.member_failed(rm, h, m);
        if (loss_sum_out) loss_sum_out[m] = o.loss_sum;
        if (loss_last_out) loss_last_out[m] = o.loss_last;
    }
    if (!bad.empty()) return g.refuse(FNN_ERR_RANGE, "feature id outside [-1, n_rows) in model(s) " + bad);
    return FNN_OK;
}

// One mini-batch step of several models on one feed (the kernels: k_fm_step_*), as a GroupCall: every launch on hs[0]'s stream,
// the call's argument array through hs[0]'s step_ring.  Each member's entry is its plan_step(), the plan the solo step launches.
int fm_train_step_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const float* y, int B,
                        const float* lr, const float* lambda, const int* reduce_mean, float* const* p_out, float* loss_out)
{
    FmGroup g("fm_train_step_multi", hs, n_models, FM_STEP_MAX_MODELS, g_fm_err);
    if (!hs || !lr || !lambda) return g.refuse(FNN_ERR_ARG, "null hs, lr or lambda");
    int rc = g.check_list("two updates would race on one table");
    if (rc != FNN_OK) return rc;
    if (!ids || !y) return g.refuse(FNN_ERR_ARG, "null ids or y");
    if (B < 1) return g.refuse(FNN_ERR_ARG, "B must be in [1, max_batch]");
    for (int m = 0; m < n_models; ++m) if (B > hs[m]->Bmax) return g.refuse(FNN_ERR_ARG, g.at("B must be in [1, max_batch]", m));
    for (int m = 0; m < n_models; ++m) {                              // fm_train_step_w's own expressions
        const fm_handle* h = hs[m];
        if (h->opt == FM_OPT_SGD && (!(lr[m] * lambda[m] < 1.0f) || lambda[m] < 0.f)) return g.refuse(FNN_ERR_ARG, g.at("need 0 <= lr * lambda < 1", m));
        if (h->opt != FM_OPT_SGD && (!(lambda[m] >= 0.f) || !(lr[m] > 0.f))) return g.refuse(FNN_ERR_ARG, g.at("Adam / FTRL need lr > 0 and lambda >= 0", m));
    }
    rc = check_tables(g);
    if (rc != FNN_OK) return rc;
    fm_handle* h0 = g.h0;
    if (n_models == 1) {       // nothing to share: the solo step itself, without the argument copy (15 us in front of a 27 us step)
        const int rs = fm_train_step_w(h0, ids, wts, y, B, lr[0], lambda[0], reduce_mean ? reduce_mean[0] : 0, p_out ? p_out[0] : nullptr, loss_out);
        if (rs == FNN_ERR_RANGE) g.refuse(rs, "feature id outside [-1, n_rows) in model(s) 0");
        return rs;
    }
    rc = g.enter();
    if (rc != FNN_OK) return rc;
    const hipStream_t st = h0->st;
    const int F = h0->F, M = n_models;
    if (!h0->step_pack) MHK(h0, hipMalloc((void**)&h0->step_pack, FM_STEP_MAX_MODELS * sizeof(StepPack)));
    size_t slot = 0;
    rc = ring_take(h0, h0->step_ring, (size_t)M, &slot);
    if (rc != FNN_OK) return rc;
    StepArg* a = h0->step_ring.at_host<StepArg>(slot);
    const StepArg* d = h0->step_ring.at_dev<StepArg>(slot);
    StepPack* pack = loss_out ? h0->step_pack : nullptr;

    // grouping classes: equal n_rows and equal shared-rows mode; the class's first model lends rec, skeys and the marks
    struct Cls { fm_handle* lead; int stamp; };
    std::vector<Cls> cls;
    std::vector<int> cls_of(M);
    for (int m = 0; m < M; ++m)
        cls_of[m] = (int)class_index(cls, Cls{hs[m], 0}, [](const Cls& a, const Cls& b) {
            return a.lead->n_rows == b.lead->n_rows && a.lead->shared == b.lead->shared; });
    // the classes with the first one's key width have their rank merge in launch 2; the others a launch of their own
    std::vector<int> order;                                           // classes, the riders first
    for (int c = 0; c < (int)cls.size(); ++c) if (cls[c].lead->key64 == cls[0].lead->key64) order.push_back(c);
    const int nride = (int)order.size();
    for (int c = 0; c < (int)cls.size(); ++c) if (cls[c].lead->key64 != cls[0].lead->key64) order.push_back(c);
    std::vector<SortArgs> sorts(cls.size());
    for (int i = 0; i < (int)order.size(); ++i) {
        Cls& k = cls[order[i]];
        fm_handle* h = k.lead;
        SortArgs so{ids, B, F, h->n_rows, h->rg.rec, h->rg.owner_cnt, 4 * F, h->skeys};
        so.merge4 = h->sort_merge4;
        launch_sort_runs(st, h->key64, so);                           // launch 1
        so.nblk = 16 * F;
        if (h->shared) {
            so.tag_first = h->tag_first; so.tag_shared = h->tag_shared;
            so.stamp = k.stamp = on_stream(h, st, [&] { return fm_next_stamp(h); });
        }
        sorts[i] = so;
        a[i].so = so;
    }
    MHK(h0, hipGetLastError());

    const bool wt = fm_wt_env();
    auto lay_of = [](const fm_handle* h) { return !h->wide ? 0 : h->rw <= 64 ? 1 : 2; };          // launch_fwd_nw's choice of kernel
    auto form_of = [](const fm_handle* h) { return h->wide ? 2 : h->shared ? 1 : 0; };              // level 1 / 2: narrow, narrow shared, wide
    int fcnt[3] = {0, 0, 0}, scnt[3] = {0, 0, 0}, ffirst[3], sfirst[3], fpos[3], spos[3], nb1max[3] = {0, 0, 0};
    for (int m = 0; m < M; ++m) { ++fcnt[lay_of(hs[m])]; ++scnt[form_of(hs[m])]; }
    ffirst[0] = sfirst[0] = 0;
    for (int c = 1; c < 3; ++c) { ffirst[c] = ffirst[c - 1] + fcnt[c - 1]; sfirst[c] = sfirst[c - 1] + scnt[c - 1]; }
    for (int c = 0; c < 3; ++c) { fpos[c] = ffirst[c]; spos[c] = sfirst[c]; }
    std::vector<float> lr_step(M);
    for (int m = 0; m < M; ++m) {                                     // plan, store into a[m], bucket by layout / form
        fm_handle* h = hs[m];
        const Cls& k = cls[cls_of[m]];
        const StepPlan p = plan_step(h, ids, wts, y, B, lr[m], lambda[m], reduce_mean ? reduce_mean[m] : 0, p_out ? p_out[m] : nullptr, wt,
                                     k.lead, k.stamp, SCAT1_HALF, SCAT2_WAVE);
        a[m].a = p.a; a[m].sa = p.sa; a[m].t = p.t; a[m].nb1 = p.nb1;
        lr_step[m] = p.lr_step;
        a[m].own_marks = nullptr; a[m].own_stamp = 0;
        if (h->shared && h != k.lead) { a[m].own_marks = h->tag_shared; a[m].own_stamp = on_stream(h, st, [&] { return fm_next_stamp(h); }); }
        a[m].pack = pack ? pack + m : nullptr;
        a[fpos[lay_of(h)]++].fcls = m;
        a[spos[form_of(h)]++].scls = m;
        nb1max[form_of(h)] = std::max(nb1max[form_of(h)], p.nb1);
    }
    rc = ring_send(h0, h0->step_ring, slot, (size_t)M);
    if (rc != FNN_OK) return rc;
    for (int i = nride; i < (int)order.size(); ++i) {                 // the other key width: the plain rank merge
        const SortArgs& so = sorts[i];
        if (cls[order[i]].lead->key64) hipLaunchKernelGGL((k_sortB<unsigned long long>), dim3(so.nblk), dim3(256), sort_lds_bytes<unsigned long long>(), st, so);
        else hipLaunchKernelGGL((k_sortB<unsigned>), dim3(so.nblk), dim3(256), sort_lds_bytes<unsigned>(), st, so);
    }
    int ride = nride;                                                 // launch 2: the merges ride in the first layout present
    for (int c = 0; c < 3; ++c) {
        if (!fcnt[c]) continue;
        const int tiles = (B + (c == 2 ? 8 : 16) - 1) / (c == 2 ? 8 : 16);
        if (cls[0].lead->key64) launch_step_fwd<unsigned long long>(st, F, wts != nullptr, c, d, ride, 16 * F, ffirst[c], fcnt[c], tiles);
        else launch_step_fwd<unsigned>(st, F, wts != nullptr, c, d, ride, 16 * F, ffirst[c], fcnt[c], tiles);
        ride = 0;
    }
    MHK(h0, hipGetLastError());
    if (scnt[0]) hipLaunchKernelGGL(k_fm_step_scat1<false>, dim3(nb1max[0], scnt[0]), dim3(256), 0, st, d, sfirst[0]);      // launch 3
    if (scnt[1]) hipLaunchKernelGGL(k_fm_step_scat1<true>, dim3(nb1max[1], scnt[1]), dim3(256), 0, st, d, sfirst[1]);
    if (scnt[2]) hipLaunchKernelGGL(k_fm_step_scatw1, dim3(nb1max[2], scnt[2]), dim3(256), 0, st, d, sfirst[2]);
    if (scnt[0]) hipLaunchKernelGGL(k_fm_step_scat2_tail<false>, dim3(1 + 256, scnt[0]), dim3(256), 0, st, d, sfirst[0]);   // launch 4
    if (scnt[1]) hipLaunchKernelGGL(k_fm_step_scat2_tail<true>, dim3(1 + 256, scnt[1]), dim3(256), 0, st, d, sfirst[1]);
    if (scnt[2]) hipLaunchKernelGGL(k_fm_step_scatw2_tail, dim3(1 + 256, scnt[2]), dim3(256), 0, st, d, sfirst[2]);
    MHK(h0, hipGetLastError());
    for (int m = 0; m < M; ++m) {                                     // Adam / FTRL: the dense pass; SGD: the fold where it is due
        fm_handle* h = hs[m];
        if (h->opt != FM_OPT_SGD) {
            on_stream(h, st, [&] { launch_opt_pass(h, lambda[m], lr_step[m]); return 0; });
            MHK(h0, hipGetLastError());
        } else if (h->scale < 5.96e-8 || h->scale > 1.0) {
            const int rf = on_stream(h, st, [&] { return fold_scale(h); });
            if (rf != FNN_OK) return g.member_failed(rf, h, m);
        }
    }
    rc = g.leave();
    if (rc != FNN_OK || !loss_out) return rc;
    std::vector<StepPack> hp(M);
    MHK(h0, hipMemcpyAsync(hp.data(), pack, (size_t)M * sizeof(StepPack), hipMemcpyDeviceToHost, st));
    MHK(h0, hipStreamSynchronize(st));
    std::string bad;
    for (int m = 0; m < M; ++m) {
        loss_out[m] = hp[m].loss;
        if (hp[m].flag) eval_list_add(bad, m);
    }
    if (!bad.empty()) return g.refuse(FNN_ERR_RANGE, "feature id outside [-1, n_rows) in model(s) " + bad);
    return FNN_OK;
}

const char* fm_online_form(const fm_handle*) { return "plain"; }

int fm_predict(fm_handle* h, const int32_t* ids, int B, float* p_out) { return fm_predict_w(h, ids, nullptr, B, p_out); }

int fm_predict_w(fm_handle* h, const int32_t* ids, const float* wts, int B, float* p_out)
{
    if (!h || !ids || !p_out) return FNN_ERR_ARG;
    if (B < 1 || B > h->Bmax) MFAIL(h, FNN_ERR_ARG, "B must be in [1, max_batch]");
    if (!h->table16) MFAIL(h, FNN_ERR_STATE, "fm_set_table has not been called");
    MHK(h, hipSetDevice(h->dev));
    return fm_forward(h, ids, wts, B, p_out);
}

int fm_set_optimizer(fm_handle* h, int optimizer, float beta1, float beta2, float eps)
{
    if (!h) return FNN_ERR_ARG;
    if (optimizer != FM_OPT_SGD && optimizer != FM_OPT_ADAM && optimizer != FM_OPT_FTRL) MFAIL(h, FNN_ERR_ARG, "bad optimizer");
    if (optimizer == FM_OPT_ADAM && !(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f))
        MFAIL(h, FNN_ERR_ARG, "Adam needs 0 <= beta1, beta2 < 1 and eps > 0");
    MHK(h, hipSetDevice(h->dev));
    const int rc = fold_scale(h);                                  // the pending SGD decay goes into the rows first
    if (rc != FNN_OK) return rc;
    MHK(h, hipStreamSynchronize(h->st));
    h->opt = optimizer;
    if (optimizer == FM_OPT_ADAM) { h->beta1 = beta1; h->beta2 = beta2; h->eps = eps; }
    return init_opt_state(h);
}

int fm_get_opt_state(fm_handle* h, float* s0, float* s1, float* sb, int64_t* t)
{
    if (!h) return FNN_ERR_ARG;
    if (h->opt == FM_OPT_SGD) MFAIL(h, FNN_ERR_STATE, "plain SGD keeps no optimiser state");
    if (!h->table16) MFAIL(h, FNN_ERR_STATE, "fm_set_table has not been called");
    MHK(h, hipSetDevice(h->dev)); MHK(h, hipStreamSynchronize(h->st));
    const size_t n = (size_t)h->n_rows * h->K * 4;
    if (s0) MHK(h, hipMemcpy(s0, h->s0, n, hipMemcpyDeviceToHost));
    if (s1) MHK(h, hipMemcpy(s1, h->s1, n, hipMemcpyDeviceToHost));
    if (sb) MHK(h, hipMemcpy(sb, h->sb, 8, hipMemcpyDeviceToHost));
    if (t) *t = h->t;
    return FNN_OK;
}

int fm_set_shared_rows(fm_handle* h, int on)
{
    if (!h) return FNN_ERR_ARG;
    MHK(h, hipSetDevice(h->dev));
    const bool want = on != 0;
    if (want == h->shared) return FNN_OK;
    MHK(h, hipStreamSynchronize(h->st));
    h->shared = want;
    h->step_stamp = 0;                                            // no step has run under this setting
    if (want && h->table16 && !h->tag_first) return alloc_tags(h);
    return FNN_OK;
}

int fm_count_shared_rows(fm_handle* h, int64_t* n_out)
{
    if (!h || !n_out) return FNN_ERR_ARG;
    if (!h->shared) MFAIL(h, FNN_ERR_STATE, "fm_set_shared_rows is off");
    if (!h->step_stamp) MFAIL(h, FNN_ERR_STATE, "no training step has run since fm_set_shared_rows / fm_set_table");
    MHK(h, hipSetDevice(h->dev));
    MHK(h, hipMemsetAsync(h->mark_cnt, 0, 8, h->st));
    const int64_t nb = (h->n_rows + 255) / 256;
    hipLaunchKernelGGL(k_fm_count_marks, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, h->st, h->tag_shared, h->n_rows, h->step_stamp,
                       h->mark_cnt);
    MHK(h, hipGetLastError());
    unsigned long long c = 0;
    MHK(h, hipMemcpyAsync(&c, h->mark_cnt, 8, hipMemcpyDeviceToHost, h->st));
    MHK(h, hipStreamSynchronize(h->st));
    *n_out = (int64_t)c;
    return FNN_OK;
}

int fm_eval(fm_handle* h, const int32_t* ids, const int32_t* y, int64_t N, double* auc, double* rmse, double* logloss)
{
    return fm_eval_w(h, ids, nullptr, y, N, auc, rmse, logloss);
}

int fm_eval_w(fm_handle* h, const int32_t* ids, const float* wts, const int32_t* y, int64_t N, double* auc, double* rmse, double* logloss)
{
    if (!h || !ids || !y || N < 1) return FNN_ERR_ARG;
    if (!h->table16) MFAIL(h, FNN_ERR_STATE, "fm_set_table has not been called");
    MHK(h, hipSetDevice(h->dev));
    float* p_d = nullptr;
    MHK(h, hipMalloc((void**)&p_d, (size_t)N * 4));
    for (int64_t lo = 0; lo < N; lo += h->Bmax) {
        const int B = (int)(N - lo < h->Bmax ? N - lo : h->Bmax);
        const int rc = fm_forward(h, ids + lo * h->F, wts ? wts + lo * h->F : nullptr, B, p_d + lo);
        if (rc != FNN_OK) { hipFree(p_d); return rc; }
    }
    double out[4] = {0, 0, 0, 0};
    std::string merr;
    const int mrc = device_metrics(h->st, p_d, y, N, out, merr);
    hipFree(p_d);
    if (mrc == -1) MFAIL(h, FNN_ERR_HIP, merr);
    if (auc) *auc = out[0];
    if (rmse) *rmse = out[1];
    if (logloss) *logloss = out[2];
    const int rc = fm_sync(h);
    if (rc != FNN_OK) return rc;
    if (mrc == -2 || mrc == -3) MFAIL(h, FNN_ERR_RANGE, merr);
    return FNN_OK;
}

// Several models, one test feed (fm_predict_multi, fm_eval_multi), as GroupCalls: every launch on hs[0]'s stream, the argument
// array of a group through hs[0]'s eval_ring.  A handle may be listed twice: reading is not a race.
namespace {

// what both calls refuse after the list itself
int eval_check(const FmGroup& g, const int32_t* ids, bool need_y, const int32_t* y, int64_t N)
{
    if (!ids || (need_y && !y)) return g.refuse(FNN_ERR_ARG, need_y ? "null ids or y" : "null ids");
    if (N < 1 || N > ((int64_t)1 << 30)) return g.refuse(FNN_ERR_ARG, "N must be in [1, 2^30]");
    return check_tables(g);
}

// The predictions of g models on the N lines, p[m] (nullable) each: the argument array into the ring, then one launch per layout
// class present.  *dev_args: where the group's arguments are on the device (k_fm_eval_flags reads them again).
int eval_forward(fm_handle* h0, fm_handle* const* hs, int g, const int32_t* ids, const float* wts, int64_t N, float* const* p,
                 const EvalArg** dev_args)
{
    size_t slot = 0;
    int rc = ring_take(h0, h0->eval_ring, (size_t)g, &slot);
    if (rc != FNN_OK) return rc;
    EvalArg* a = h0->eval_ring.at_host<EvalArg>(slot);
    const EvalArg* d = h0->eval_ring.at_dev<EvalArg>(slot);
    auto cls_of = [](const fm_handle* h) { return !h->wide ? 0 : h->rw <= 64 ? 1 : 2; };   // launch_fwd_nw's choice of kernel
    int cnt[3] = {0, 0, 0}, first[3], pos[3];
    for (int m = 0; m < g; ++m) ++cnt[cls_of(hs[m])];
    first[0] = 0; first[1] = cnt[0]; first[2] = cnt[0] + cnt[1];
    for (int c = 0; c < 3; ++c) pos[c] = first[c];
    const bool wt = fm_wt_env();
    for (int m = 0; m < g; ++m) {
        a[m].a = predict_args(hs[m], ids, wts, (int)N, p[m], wt);
        a[pos[cls_of(hs[m])]++].cls = m;
    }
    const hipStream_t st = h0->st;
    rc = ring_send(h0, h0->eval_ring, slot, (size_t)g);
    if (rc != FNN_OK) return rc;
    const char* order = getenv("FM_EVAL_ORDER");                  // "model": the model is the fast index of the grid; default: the tile
    const int model_fast = order && !strcmp(order, "model");
    for (int c = 0; c < 3; ++c) {
        if (!cnt[c]) continue;
        const int epb = c == 2 ? 8 : 16;                          // examples per workgroup: 256 / L, 16 on the narrow path
        const int64_t tiles = (N + epb - 1) / epb, total = tiles * cnt[c];
        const int64_t gx = total < (1 << 22) ? total : (1 << 22);
        const dim3 grid((unsigned)gx, (unsigned)((total + gx - 1) / gx));
        switch ((h0->F + 15) / 16) {
        case 1: launch_multi_n<1>(wts != nullptr, st, c, grid, d, first[c], cnt[c], tiles, model_fast); break;
        case 2: launch_multi_n<2>(wts != nullptr, st, c, grid, d, first[c], cnt[c], tiles, model_fast); break;
        case 3: launch_multi_n<3>(wts != nullptr, st, c, grid, d, first[c], cnt[c], tiles, model_fast); break;
        default: launch_multi_n<4>(wts != nullptr, st, c, grid, d, first[c], cnt[c], tiles, model_fast); break;
        }
        MHK(h0, hipGetLastError());
    }
    *dev_args = d;
    return FNN_OK;
}

}  // namespace

int fm_predict_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, int64_t N, float* const* p_out)
{
    FmGroup g("fm_predict_multi", hs, n_models, FM_EVAL_MAX_MODELS, g_fm_err);
    int rc = g.check_list(nullptr);
    if (rc == FNN_OK) rc = eval_check(g, ids, false, nullptr, N);
    if (rc != FNN_OK) return rc;
    if (!p_out) return g.refuse(FNN_ERR_ARG, "null p_out");
    rc = g.enter();
    if (rc != FNN_OK) return rc;
    const EvalArg* d = nullptr;
    rc = eval_forward(g.h0, hs, n_models, ids, wts, N, p_out, &d);
    const int rj = g.leave();
    return rc != FNN_OK ? rc : rj;
}

int fm_eval_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const int32_t* y, int64_t N,
                  double* auc, double* rmse, double* logloss, int* status)
{
    FmGroup g("fm_eval_multi", hs, n_models, FM_EVAL_MAX_MODELS, g_fm_err);
    int rc = g.check_list(nullptr);
    if (rc == FNN_OK) rc = eval_check(g, ids, true, y, N);
    if (rc != FNN_OK) return rc;
    fm_handle* h0 = g.h0;
    // the models of a group share one scratch allocation, the call's own: as many as fit under the cap, one at the least
    const int G = eval_group_size(n_models, N, "FM_EVAL_SCRATCH_BYTES");
    rc = g.enter();
    if (rc != FNN_OK) return rc;
    const hipStream_t st = h0->st;
    char* scratch = nullptr;
    MHK(h0, hipMalloc((void**)&scratch, EvalScratch::bytes(G, N)));
    const EvalArg* d = nullptr;                                       // the group's arguments on the device, from its forward to its flags
    const EvalForward forward = [&](int g0, int n, float* const* p) { return eval_forward(h0, hs + g0, n, ids, wts, N, p, &d); };
    const EvalFlags flags = [&](int, int n, int* flags_d) {
        hipLaunchKernelGGL(k_fm_eval_flags, dim3(1), dim3(256), 0, st, d, n, flags_d);
        MHK(h0, hipGetLastError());
        return FNN_OK;
    };
    EvalFound found;
    rc = eval_groups(st, n_models, G, y, N, scratch, forward, flags, EvalOut{auc, rmse, logloss, status, nullptr}, found, h0->err);
    const int rj = g.leave();
    hipFree(scratch);                                                 // (after an error eval_groups has drained the stream)
    if (rc != FNN_OK) return rc;
    if (rj != FNN_OK) return rj;
    const std::string msg = eval_verdict(found.bad, found.range, found.n_pos, N, "[-1, n_rows)");
    return msg.empty() ? FNN_OK : g.refuse(FNN_ERR_RANGE, msg);
}

}  // extern "C"
