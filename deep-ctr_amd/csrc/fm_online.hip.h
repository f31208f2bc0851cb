// fm_online.hip.h -- FM / LR pre-training on the reference's ONLINE schedule (python/ipinyou.py:129-140 builds both models with
// batch_size = 1 and :167-173 runs one step per line): fm_train_online of include/fm_hip.h.  One persistent workgroup walks the
// examples of a launch in line order; example n is trained on the parameters examples 0..n-1 left.  The work is a dependence
// chain through b and the rows, so there is nothing for a second workgroup to do without breaking that order: the rate of this
// kernel is a latency figure (one workgroup on a 256-CU part), not a share of any roofline.
//
// A step is fm_train_step_w at B = 1 (fm_hip.h, "Arithmetic"): e_f = (scale x_f) row(id_f), S_l = sum_f e_f[l],
// yhat = b + sum_f e_f[0] + 1/2 sum_l (S_l^2 - sum_f e_f[l]^2), delta = sigmoid(yhat) - y, and under the lazy decay scale
// stored <- stored - (lr / scale_new) g with g[0] = delta x_f, g[l] = delta x_f (S_l - e_f[l]); b <- b (1 - lr lambda) - lr delta.
// The kernel carries the scale as a double and multiplies it by `dec` = 1 - (double)lr (double)lambda once per example; the
// host advances its copy by the same multiplications, so the two agree bit for bit and nothing is read back.
//
// Per example, 256 threads and four barriers:
//   gather   thread i owns row pieces i, i + 256, .. of the line's F * ceil(K / 4) 16-byte pieces (at most 8 of them, F = 64 and
//            k = 128): every load is issued before the first is used; the pieces go to LDS and stay in the thread's registers
//   sums     thread (q, g) = (tid & 31, tid >> 5) sums piece column q over the fields g, g + 8, ..; wave 0 adds the eight partial
//            sums in group order, lane 0 takes yhat, p, delta, the loss and the new b
//   update   the owner of a piece updates it from its registers and stores it.  A row under several columns of the line is
//            stored once, by its FIRST column, with the sum (f64, in column order) of every column's contribution: wave 0 links
//            the columns that hold one row while it stages the ids (s_own / s_next), a line ahead of their use.
// Ids, weights and labels do not depend on earlier examples: wave 0 requests them two examples ahead and stages them (range
// check, absent -> weight 0, the column links) into the other of two LDS buffers while the update of the current example runs.
// The __syncthreads() that ends an example stands between its row stores and the next example's row loads (one workgroup, one
// CU, one L1: workgroup-scope release / acquire, as in the online RBM and DAE trainers).  No float atomics; plain vector stores.
//
// Several models on one feed (fm_train_online_multi): the chains of different models are independent, so k_fm_online_multi is a
// grid of them, a workgroup per model, each running the same body on its own Args.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fm_online {

struct Out { double loss_sum; float loss_last; float pad; };     // accumulated over the launches of one call

struct Args {
    const int32_t* ids; const float* wts; const float* y;         // this launch's examples: [N, F], [N, F] or null, [N]
    int64_t N; int F, K, rw;                                      // rw: the row stride in floats (16, or rup(k, 4) for k >= 17)
    float* table; int64_t n_rows; float* b;
    double scale, dec;                                            // the lazy scale before example 0; 1 - (double)lr (double)lambda
    float lr, lambda; float* p_out; int* err; Out* out;
};

constexpr int MAXF = 64, MAXQ = 32, NPT = MAXF * MAXQ / 256;      // fields, 16-byte pieces of a row, pieces per thread

// Args' pointers as the body uses them: to global memory, said in the type.  k_fm_online's are kernel arguments, which the compiler
// knows to be global; k_fm_online_multi reads them from memory, where a plain pointer is a generic one and every access through
// it a flat instruction.  A row piece is an ext-vector value from its load to its last use (a 16-byte load of an address-space
// pointer yields one; copying it into a float4 would put a wait behind every load).
#define FM_ONLINE_GLOBAL __attribute__((address_space(1)))
typedef float v4f __attribute__((ext_vector_type(4)));

// The examples of one launch for one model: the whole workgroup calls it once.  k_fm_online and k_fm_online_multi are this body
// and nothing else, so what a model computes does not depend on which of the two runs it.
//
// Roundings are pinned in the source.  The library is built with -ffp-contract=fast, under which the backend decides per
// instruction whether a product and the sum that takes it become one FMA -- and __fmul_rn is a plain product to it.  It used to
// decide: of the four lanes of S - r s in the update three were FMAs and one was not, and which one depended on how the code
// around it was laid out, so any edit here could move the last bit of a row.  Contraction is therefore OFF in this body, and every
// fused operation is an fmaf / fma that says so.  Which are fused is what the kernel computed before the pin, kept so that
// fm_train_online's bits did not change: marked "fused" below; everything else rounds after every operation.
__device__ __forceinline__ void online_body(const Args& a)
{
#pragma clang fp contract(off)
    __shared__ v4f s_raw[MAXF * MAXQ];                            // the line's row pieces as stored, [f][nq]
    __shared__ float4 s_pS[8][MAXQ], s_pq[8][MAXQ], s_S[MAXQ];    // partial sums of e and e^2 per field group; the field sums
    __shared__ float s_lin[8], s_delta;
    __shared__ int s_id[2][MAXF], s_next[2][MAXF], s_own[2][MAXF];
    __shared__ float s_x[2][MAXF];
    const int tid = threadIdx.x, F = a.F, K = a.K, nq = (K + 3) >> 2, P = F * nq;
    const int q = tid & 31, g = tid >> 5;
    const FM_ONLINE_GLOBAL int32_t* const g_ids = (const FM_ONLINE_GLOBAL int32_t*)a.ids;
    const FM_ONLINE_GLOBAL float* const g_wts = (const FM_ONLINE_GLOBAL float*)a.wts;
    const FM_ONLINE_GLOBAL float* const g_y = (const FM_ONLINE_GLOBAL float*)a.y;
    FM_ONLINE_GLOBAL float* const g_table = (FM_ONLINE_GLOBAL float*)a.table;
    FM_ONLINE_GLOBAL float* const g_b = (FM_ONLINE_GLOBAL float*)a.b;
    FM_ONLINE_GLOBAL float* const g_p = (FM_ONLINE_GLOBAL float*)a.p_out;
    FM_ONLINE_GLOBAL Out* const g_out = (FM_ONLINE_GLOBAL Out*)a.out;
    FM_ONLINE_GLOBAL int* const g_err = (FM_ONLINE_GLOBAL int*)a.err;
    const float b_dec = fmaf(-a.lr, a.lambda, 1.0f);              // fused: 1 - lr lambda of the bias
    int pf[NPT], pq[NPT];                                         // the thread's pieces: field and piece column
#pragma unroll
    for (int j = 0; j < NPT; ++j) { const int i = tid + 256 * j; pf[j] = i < P ? i / nq : -1; pq[j] = i < P ? i % nq : 0; }

    // wave 0, lane = column: the ids and weights of the example two ahead, requested here and checked when they are staged
    int r_id = -1; float r_x = 0.f;
    auto fetch = [&](const int64_t n) {
        r_id = -1; r_x = 1.f;
        if (tid < F && n < a.N) {
            r_id = g_ids[(size_t)n * F + tid];
            if (a.wts) r_x = g_wts[(size_t)n * F + tid];
        }
    };
    // stage the fetched line into buffer `buf`: an id outside [-1, n_rows) is reported and absent, an absent field has weight 0
    // whatever was loaded, and columns that hold one row are linked: s_own = the first of them, s_next = the next one or -1
    auto stage = [&](const int buf) {
        int id = r_id;
        if (id < -1 || (int64_t)id >= a.n_rows) { __hip_atomic_fetch_or(g_err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); id = -1; }
        const float x = id >= 0 ? r_x : 0.f;
        int next = -1, own = id >= 0;
        for (int j = 0; j < F; ++j) {
            const int idj = __builtin_amdgcn_readlane(id, j);
            const bool same = id >= 0 && idj == id;
            if (same && j < tid) own = 0;
            if (same && j > tid && next < 0) next = j;
        }
        if (tid < F) { s_id[buf][tid] = id; s_x[buf][tid] = x; s_next[buf][tid] = next; s_own[buf][tid] = own; }
    };

    double scale = a.scale, loss_sum = 0.0;
    float b = 0.f, loss_last = 0.f, y_cur = 0.f, y_next = 0.f;
    if (tid == 0) { b = *g_b; loss_sum = g_out->loss_sum; loss_last = g_out->loss_last; y_cur = g_y[0]; if (a.N > 1) y_next = g_y[1]; }
    if (tid < 64) { fetch(0); stage(0); fetch(1); }
    __syncthreads();

    for (int64_t n = 0; n < a.N; ++n) {
        const int buf = (int)(n & 1);
        const float scale_f = (float)scale;                       // e = (scale x) row at the scale before this example's decay
        scale *= a.dec;
        const double coef = (double)a.lr / scale;
        // gather: every load first
        v4f v[NPT];
        int id[NPT];
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            v[j] = v4f{0.f, 0.f, 0.f, 0.f};
            id[j] = -1;
            if (pf[j] >= 0) {
                id[j] = s_id[buf][pf[j]];
                if (id[j] >= 0) v[j] = *reinterpret_cast<const FM_ONLINE_GLOBAL v4f*>(g_table + (size_t)id[j] * a.rw + 4 * pq[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < NPT; ++j) if (pf[j] >= 0) s_raw[tid + 256 * j] = v[j];
        __syncthreads();
        // sums over the fields g, g + 8, ..; column 0 of a row is w_f: it goes to the linear term and not into S / sq
        {
            float4 S = make_float4(0.f, 0.f, 0.f, 0.f), sq = S;
            float lin = 0.f;
            if (q < nq) {
                for (int f = g; f < F; f += 8) {
                    const float s = scale_f * s_x[buf][f];
                    const v4f r = s_raw[f * nq + q];
                    v4f e = r * s;
                    if (q == 0) { lin = fmaf(r.x, s, lin); e.x = 0.f; }                   // fused
                    S.x += e.x; S.y += e.y; S.z = fmaf(r.z, s, S.z); S.w = fmaf(r.w, s, S.w);    // z and w fused, x and y not
                    sq.x = fmaf(e.x, e.x, sq.x); sq.y = fmaf(e.y, e.y, sq.y); sq.z = fmaf(e.z, e.z, sq.z); sq.w = fmaf(e.w, e.w, sq.w);
                }
            }
            s_pS[g][q] = S; s_pq[g][q] = sq;
            if (q == 0) s_lin[g] = lin;
        }
        __syncthreads();
        if (tid < 64) {
            float4 S = make_float4(0.f, 0.f, 0.f, 0.f), sq = S;
            float lin = 0.f;
#pragma unroll
            for (int gg = 0; gg < 8; ++gg) {
                const float4 ps = s_pS[gg][q], pp = s_pq[gg][q];
                S.x += ps.x; S.y += ps.y; S.z += ps.z; S.w += ps.w;
                sq.x += pp.x; sq.y += pp.y; sq.z += pp.z; sq.w += pp.w;
                lin += s_lin[gg];
            }
            // yhat = b + sum_f w_f + 1/2 (sum_l S_l^2 - sum_f sum_l v_f[l]^2)                     (python/FM.py:56-63)
            float part = 0.5f * ((fmaf(S.x, S.x, -sq.x) + fmaf(S.y, S.y, -sq.y)) + (fmaf(S.z, S.z, -sq.z) + fmaf(S.w, S.w, -sq.w)));
            if (tid >= 32) part = 0.f;
            if (tid == 0) part += lin;
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) part += __shfl_xor(part, o, 32);
            if (tid < 32) s_S[tid] = S;
            if (tid == 0) {
                const float z = b + part;
                const float p = 1.0f / (1.0f + expf(-z));
                const float delta = p - y_cur;
                loss_last = fmaf(-y_cur, z, fmaxf(z, 0.f)) + log1pf(expf(-fabsf(z)));    // fused
                loss_sum += (double)loss_last;
                s_delta = delta;
                b = fmaf(b_dec, b, -(a.lr * delta));                                      // fused
                if (a.p_out) g_p[n] = p;
            }
        }
        __syncthreads();
        // the next example's line into the other buffer (nobody reads that one before the barrier below), the one after it requested
        if (tid < 64 && n + 1 < a.N) {
            stage(buf ^ 1);
            fetch(n + 2);
            if (tid == 0) { y_cur = y_next; if (n + 2 < a.N) y_next = g_y[n + 2]; }
        }
        // update: d yhat / d w_f = x_f ; d yhat / d v_f[l] = x_f (S_l - e_f[l]); the columns of one row summed into its first
        const float delta = s_delta;
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            if (pf[j] < 0 || id[j] < 0 || !s_own[buf][pf[j]]) continue;
            const int c = 4 * pq[j];
            const float4 S = s_S[pq[j]];
            const v4f r = v[j];
            double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
            for (int f = pf[j]; f >= 0; f = s_next[buf][f]) {
                const float x = s_x[buf][f], s = scale_f * x, dx = delta * x;
                // S_l - e_f[l]: fused in lanes x, z and w, lane y takes the rounded product
                g0 += (double)(c == 0 ? dx : (c < K ? dx * fmaf(-r.x, s, S.x) : 0.f));
                g1 += (double)(c + 1 < K ? dx * (S.y - r.y * s) : 0.f);
                g2 += (double)(c + 2 < K ? dx * fmaf(-r.z, s, S.z) : 0.f);
                g3 += (double)(c + 3 < K ? dx * fmaf(-r.w, s, S.w) : 0.f);
            }
            const v4f w = {(float)fma(-coef, g0, (double)r.x), (float)fma(-coef, g1, (double)r.y),      // fused
                           (float)fma(-coef, g2, (double)r.z), (float)fma(-coef, g3, (double)r.w)};
            *reinterpret_cast<FM_ONLINE_GLOBAL v4f*>(g_table + (size_t)id[j] * a.rw + 4 * pq[j]) = w;
        }
        __syncthreads();          // the row stores are visible to the workgroup before the next example's loads
    }
    if (tid == 0) { *g_b = b; g_out->loss_sum = loss_sum; g_out->loss_last = loss_last; }
}

__global__ __launch_bounds__(256) void k_fm_online(const Args a) { online_body(a); }

// fm_train_online_multi: workgroup m is model m's chain, args[m] its arguments (read once, here).  The models share the feed and
// nothing else -- every table, b, error flag and Out is a model's own -- so the workgroups never meet: no atomics on shared
// data, no waiting on one another; with more models than CUs the surplus workgroups queue behind the first to finish.
__global__ __launch_bounds__(256) void k_fm_online_multi(const Args* __restrict__ args)
{
    const Args a = args[blockIdx.x];
    online_body(a);
}

}  // namespace fm_online
