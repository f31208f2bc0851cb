// fnn_step_kernels.hip.h -- the three launches of a training step (gfx950 only).
//
// One pass of the reference's hot loop body (python/FNN_wnzh.py:296-306) is three kernels on one
// stream, each a union of two independent roles that run side by side on different workgroups:
//
//   k_step1 = { MLP strip kernel: gather, forward, loss, backward-data }
//   k_step2 = { weight-gradient products } U { sparse-row SGD, level 1 } U { sort runs of the NEXT batch's keys }
//   k_step3 = { slab reduce + dense SGD + shadow refresh } U { sparse-row SGD, level 2 } U { rank-merge the runs }
//
// The step is a few microseconds of math, so its cost is launches and dependent memory round
// trips; three fat launches and no cross-stream events are what that regime wants (measured:
// a 7-node hipGraph replay costs 46 us on this runtime, seven plain launches 18.5 us).
#pragma once
#include "fnn_kernels.hip.h"
#include "sparse_rows.hip.h"      // the grouping and row-update roles of launches 2 and 3

namespace fnn {

// ------------------------------------------------------------------------------------------
// step 1: MLP strips of this batch.  (At 256 VGPRs a strip workgroup fills its CU, so the sort
// roles ride on steps 2 and 3, whose workgroups are small enough to share a CU.)
// ------------------------------------------------------------------------------------------
// (WTF: mlp_body's fixed training form, -1 the generic one)
template <typename T, int C1, int C2, int CX, bool BAG, int NW = 4, int WTF = -1>
static __global__ __launch_bounds__(64 * NW) void k_step1(const MlpArgs<T> a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    mlp_body<T, C1, C2, CX, BAG, NW, WTF>(a, blockIdx.x, smem);
}

// ------------------------------------------------------------------------------------------
// step 2: run-sorts of the NEXT batch's keys  U  weight gradients  U  sparse-row SGD level 1
// ------------------------------------------------------------------------------------------
// The weight-gradient role of launch 2: block w of the role's nw = nwx * splitk workgroups -> its (tile, K slice).
// XCD-aware order: hardware block ids that differ by a multiple of 8 share an XCD (and its L2); deal the role's blocks so
// that each of the 8 classes owns a contiguous run of (tile, K slice) pairs -- one or two K slices of the operands per XCD
// instead of a little of every slice.  `aligned`: the role starts at a hardware block id that is a multiple of 8 (placement
// only: any deal computes the same slabs).
template <typename T, int WF>
__device__ __forceinline__ void wgrad_role(const WgradArgs& wa, const int nwx, int w, const int nw, const bool aligned, unsigned char* smem)
{
    if (aligned) {
        const int cls = w & 7, k = w >> 3, qd = nw >> 3, rm = nw & 7;
        w = (cls < rm ? cls * (qd + 1) : rm * (qd + 1) + (cls - rm) * qd) + k;
    }
    wgrad_body<T, WF>(wa, w % nwx, w / nwx, smem);
}
// level 1 of the sparse-row update in the form the arguments name (scat1_blocks; wide and bag rows: scatw1_body).  The group
// kernel's; k_step2 keeps the same chain written out, which keeps its code what it was to the byte (as k_step3 does for level 2).
__device__ __forceinline__ void scat1_role(const ScatArgs& sa, const int blk)
{
    if (sa.rw != SLOT) scatw1_body(sa, blk);
    else if (sa.form == SCAT1_SLOT) scat1_body(sa, blk);       // FNN_SCAT1_FORM=slot
    else if (sa.form == SCAT1_HALF) scat1h_body(sa, blk);      // FNN_SCAT1_FORM=half
    else scat1q_body(sa, blk);
}

// WF: the form of the weight-gradient role (WGRAD_LDS: WGRAD_LDS_BYTES of dynamic LDS for the whole launch; bf16 only)
template <typename T, typename KT, bool M4, int WF = WGRAD_DIRECT>
static __global__ __launch_bounds__(256) void k_step2(const SortArgs so, const WgradArgs wa, const int nwx,
                                               const int splitk, const ScatArgs sa)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int b = blockIdx.x, nw = nwx * splitk;
    if (b < so.nblk) sortA_form<KT, M4>(so, b, smem);                          // so.nblk = 4 * F or 0
    else if (b < so.nblk + nw) {
        const int w = b - so.nblk;
        wgrad_role<T, WF>(wa, nwx, w, nw, ((b ^ w) & 7) == 0, smem);
    }
    // (the scatter role's blocks dealt BEFORE the weight gradients', so that their chain starts while those are still being
    // placed, measured level: 39.06 / 38.53 / 39.01 us per step against 38.45 / 39.17 / 39.03 behind them; with the 96 blocks
    // of the half-chunk form slower, 30.8 against 29.8 -- they stay behind)
    else if (sa.rw != SLOT) scatw1_body(sa, b - so.nblk - nw);
    else if (sa.form == SCAT1_SLOT) scat1_body(sa, b - so.nblk - nw);       // FNN_SCAT1_FORM=slot
    else if (sa.form == SCAT1_HALF) scat1h_body(sa, b - so.nblk - nw);      // FNN_SCAT1_FORM=half
    else scat1q_body(sa, b - so.nblk - nw);
}

// ------------------------------------------------------------------------------------------
// step 3: slab reduce (+ L2 term) -> bucket, optional dense SGD + shadow refresh, loss sum
//         U  sparse-row SGD level 2.  UPDATE = false under data parallelism: the bucket is
//         all-reduced first and k_update applies it.
// ------------------------------------------------------------------------------------------
struct TailArgs {
    const float* slab; int splitk; size_t nw_all, nw12, nslab; float* master; float lambda1; int reg_all;
    const float* loss_t; int Ba; float* bucket; float* loss_sum; float lr; int K1p, H1p, H2p;
    void *w1, *w1t, *w2, *w2t; int nblk_red;
    float* bb0; size_t nbag, off_bag;      // bag mode: bias vector, its length (K1p) and slab offset
};

// The dense role of launch 3: block b of the role's ta.nblk_red workgroups.  The last one sums the loss (fixed-shape tree); the
// others reduce the split-K slabs into the bucket and, UPDATE, apply the step with the L2 term and refresh the shadows.
template <typename T, bool UPDATE>
__device__ __forceinline__ void dense_body(const TailArgs& ta, const int b, double (&s_sum)[16][16])
{
    if (b == ta.nblk_red - 1) {                                // loss: fixed-shape tree
        float* s_l = reinterpret_cast<float*>(&s_sum[0][0]);
        float v = 0.f;
        v = strided_sum256(ta.loss_t, ta.Ba);
        s_l[threadIdx.x] = v;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) s_l[threadIdx.x] += s_l[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) *ta.loss_sum = s_l[0];
        return;
    }
    // Dense tensors W1p, W2p: 4 consecutive elements per thread (same row, 4 columns: 16-byte slab / master
    // accesses, one 8-byte piece of the [in][out] shadow); the short tail (w3p, bag bias) one element each.
    const size_t nvec = ta.nw12 / 4;
    const int nvb = (int)((nvec + 255) / 256);
    if (b < nvb) {
        const size_t q = (size_t)b * 256 + threadIdx.x;
        if (q >= nvec) return;
        const size_t i = q * 4;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
        for (int z = 0; z < ta.splitk; ++z) {
            const float4 v = *reinterpret_cast<const float4*>(ta.slab + (size_t)z * ta.nslab + i);
            g.x += v.x; g.y += v.y; g.z += v.z; g.w += v.w;
        }
        *reinterpret_cast<float4*>(ta.bucket + i) = g;          // data term only (what data parallelism all-reduces)
        if (UPDATE) {
            float4 w = *reinterpret_cast<const float4*>(ta.master + i);
            const float l2 = ta.reg_all ? 2.0f * ta.lambda1 : 0.0f;     // L2 term (:173; only w3, b3 unless reg_all)
            w.x -= ta.lr * (g.x + l2 * w.x); w.y -= ta.lr * (g.y + l2 * w.y);
            w.z -= ta.lr * (g.z + l2 * w.z); w.w -= ta.lr * (g.w + l2 * w.w);
            *reinterpret_cast<float4*>(ta.master + i) = w;
            const size_t n1 = (size_t)ta.K1p * ta.H1p;
            const bool first = i < n1;
            const size_t j = first ? i : i - n1;
            const int ld = first ? ta.H1p : ta.H2p, kin = first ? ta.K1p : ta.H1p;
            const int r = (int)(j / ld), c = (int)(j % ld);
            T* wn = static_cast<T*>(first ? ta.w1 : ta.w2);     // [in][out]: k = column, 4 consecutive
            T* wt = static_cast<T*>(first ? ta.w1t : ta.w2t);   // [out][in]: k = row
            store4(wn + ft_off<T>(r, c, ld), w.x, w.y, w.z, w.w);
            wt[ft_off<T>(c, r, kin)] = (T)w.x; wt[ft_off<T>(c + 1, r, kin)] = (T)w.y;
            wt[ft_off<T>(c + 2, r, kin)] = (T)w.z; wt[ft_off<T>(c + 3, r, kin)] = (T)w.w;
        }
        return;
    }
    const size_t i = ta.nw12 + (size_t)(b - nvb) * 256 + threadIdx.x;
    if (i >= ta.nw_all + ta.nbag) return;
    if (i >= ta.nw_all) {               // bag bias: bb0 -= lr * sum_t delta_t  (python/SNN_RBM.py:289)
        const size_t c = i - ta.nw_all;
        float g = 0.f;
#pragma unroll 8
        for (int z = 0; z < ta.splitk; ++z) g += ta.slab[(size_t)z * ta.nslab + ta.off_bag + c * 64];
        ta.bucket[i] = g;
        if (UPDATE) ta.bb0[c] -= ta.lr * g;
        return;
    }
    const size_t src = ta.nw12 + (i - ta.nw12) * 64;            // w3p: column 0 of an [H2p][64] tile
    float g = 0.f;
#pragma unroll 8
    for (int z = 0; z < ta.splitk; ++z) g += ta.slab[(size_t)z * ta.nslab + src];
    float w = ta.master[i];
    ta.bucket[i] = g;
    if (UPDATE) {
        g += 2.0f * ta.lambda1 * w;                              // w3, b3 are always regularised (:173)
        ta.master[i] = w - ta.lr * g;
    }
}
// level 2 of the sparse-row update: block `blk` of the role's nb workgroups
__device__ __forceinline__ void scat2_role(const ScatArgs& sa, const int blk, const int nb, double (*s_sum)[16], unsigned char* smem)
{
    if (sa.rw == SLOT) {
        if (sa.form2 == SCAT2_WAVE) scat2w_body(sa, blk, nb);      // FNN_SCAT2_FORM=wave
        else scat2_body(sa, blk, nb, s_sum);
    }
    else scatw2_body(sa, blk, nb, reinterpret_cast<double*>(smem));
}

template <typename T, bool UPDATE, typename KT, bool M4>
static __global__ __launch_bounds__(256) void k_step3(const SortArgs so, const TailArgs ta, const ScatArgs sa)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double s_sum[16][16];
    if ((int)blockIdx.x < so.nblk) { sortB_form<KT, M4>(so, blockIdx.x, smem); return; }      // rank merge: 16 F or 0 WGs
    const int b = (int)blockIdx.x - so.nblk;
    if (b >= ta.nblk_red) {
        const int nb = (int)gridDim.x - so.nblk - ta.nblk_red;
        if (sa.rw == SLOT) {
            if (sa.form2 == SCAT2_WAVE) scat2w_body(sa, b - ta.nblk_red, nb);      // FNN_SCAT2_FORM=wave
            else scat2_body(sa, b - ta.nblk_red, nb, s_sum);
        }
        else scatw2_body(sa, b - ta.nblk_red, nb, reinterpret_cast<double*>(smem));
        return;
    }
    dense_body<T, UPDATE>(ta, b, s_sum);
}

// ------------------------------------------------------------------------------------------
// One step of several models on one feed (fnn_train_step_multi, fnn_bag_train_step_multi): the three launches with the model as blockIdx.y, the
// arguments of model y read from a device array, the SAME bodies on them as the solo kernels run.  The models of one launch
// agree in the kernel and its launch shape (a launch class); a model whose role counts are smaller than the grid's returns.
// Only the first member of a grouping class carries sort-role blocks (so2 / so3: nblk = 0 on the others), every member's
// ScatArgs reads that member's rec -- and, in bag mode, that member's marks of the rows under several columns (tag_shared / stamp).
// ------------------------------------------------------------------------------------------
struct GroupPack { float loss; int flag; };
template <typename T> struct GroupArg {
    MlpArgs<T> ma; int nmlp;                   // launch 1: the strips
    SortArgs so2, so3;                         // launches 2 / 3: run sorts and rank merges of the NEXT batch (first member only)
    WgradArgs wa; int nwx, splitk, nsc1;       // launch 2: tiles, K slices, level-1 workgroups
    ScatArgs sa;
    TailArgs ta; int nsc2;                     // launch 3: the dense role (ta.nblk_red workgroups), level-2 workgroups
    GroupPack* pack;                           // the call's loss and range flag of this model for one copy to the host (null: not asked)
};

// (a member's owner count is cleared here, before level 1 counts into it: the rank merge clears only the slot it fills)
// BAG: the strips of bag rows (fnn_bag_train_step_multi), what k_step1<..., true, NW> runs for each member alone
template <typename T, int C1, int C2, int CX, int NW, int WTF, bool BAG = false>
static __global__ __launch_bounds__(64 * NW) void k_gstep1(const GroupArg<T>* __restrict__ args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const GroupArg<T>& g = args[blockIdx.y];
    const MlpArgs<T> a = g.ma;
    const int nmlp = g.nmlp;
    int* const owner_cnt = g.sa.owner_cnt;
    if ((int)blockIdx.x >= nmlp) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) *owner_cnt = 0;
    mlp_body<T, C1, C2, CX, BAG, NW, WTF>(a, blockIdx.x, smem);
}

// (the grid's x extent is a multiple of 8, so that a model's blocks start on the XCD the solo launch's start on and the
// weight-gradient deal stays XCD-aware)
template <typename T, typename KT, bool M4, int WF>
static __global__ __launch_bounds__(256) void k_gstep2(const GroupArg<T>* __restrict__ args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const GroupArg<T>& g = args[blockIdx.y];
    const int b = blockIdx.x, nsort = g.so2.nblk, nwx = g.nwx, nw = nwx * g.splitk, nsc = g.nsc1;
    if (b < nsort) { const SortArgs so = g.so2; sortA_form<KT, M4>(so, b, smem); }
    else if (b < nsort + nw) {
        const WgradArgs wa = g.wa;
        const int w = b - nsort;
        wgrad_role<T, WF>(wa, nwx, w, nw, ((b ^ w) & 7) == 0, smem);
    }
    else if (b < nsort + nw + nsc) { const ScatArgs sa = g.sa; scat1_role(sa, b - nsort - nw); }
}

template <typename T, typename KT, bool M4>
static __global__ __launch_bounds__(256) void k_gstep3(const GroupArg<T>* __restrict__ args)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double s_sum[16][16];
    const GroupArg<T>& g = args[blockIdx.y];
    const int nsort = g.so3.nblk, nred = g.ta.nblk_red, nsc = g.nsc2;
    if ((int)blockIdx.x < nsort) { const SortArgs so = g.so3; sortB_form<KT, M4>(so, blockIdx.x, smem); return; }
    const int b = (int)blockIdx.x - nsort;
    if (b >= nred) {
        if (b - nred < nsc) { const ScatArgs sa = g.sa; scat2_role(sa, b - nred, nsc, s_sum, smem); }
        return;
    }
    const TailArgs ta = g.ta;
    GroupPack* const pack = g.pack;
    int* const err = g.ma.err;
    dense_body<T, true>(ta, b, s_sum);
    if (pack && b == nred - 1 && threadIdx.x == 0) { pack->loss = *ta.loss_sum; pack->flag = *err; }
}

// ------------------------------------------------------------------------------------------
// The predictions of several models on one feed (fnn_predict_multi / fnn_eval_multi): the strip kernel's generic prediction
// instance -- what step1_sel(train = false) returns for each member of the launch -- with the model as a grid dimension and
// the feed of N lines cut into FEED BATCHES of `fb_len` lines (a multiple of 256; the last one shorter), whatever the members'
// max_batch.  Strip s of the feed is strip s % (fb_len / 16) of feed batch s / (fb_len / 16): the body runs on a register copy
// of the member's arguments with ids, p_out and B moved to that feed batch, so that every index it forms (the labels' among
// them: a.y is fb_len floats long) stays below fb_len.  A line's prediction depends on that line's ids alone, so how the feed
// is cut changes no bit.  model_fast = 0: grid (strips, models), the strips of one model adjacent (they share W1 / W2 in L2);
// 1: a linear grid with the model the fast index (the models of one strip share its ids and table rows).
// ------------------------------------------------------------------------------------------
template <typename T> struct GroupPredArg { MlpArgs<T> ma; int m; };        // m: the member's place in the call's group (its range flag's)
template <typename T, int C1, int C2, int CX, int NW>
static __global__ __launch_bounds__(64 * NW) void k_gpredict(const GroupPredArg<T>* __restrict__ args, const int n_models, const int64_t N,
                                                             const int fb_len, const int64_t strip0, const int64_t n_strips, const int model_fast)
{
    extern __shared__ __align__(16) unsigned char smem[];
    int64_t s = blockIdx.x; int m = blockIdx.y;
    if (model_fast) {
        const int64_t l = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        s = l / n_models; m = (int)(l % n_models);
    }
    if (s >= n_strips) return;
    s += strip0;
    MlpArgs<T> a = args[m].ma;                                        // the whole block before anything is stored: scalar loads
    const int per = fb_len >> 4;
    const int64_t lo = s / per * fb_len;
    a.ids += lo * a.F; a.p_out += lo;
    a.B = (int)(N - lo < fb_len ? N - lo : fb_len);
    mlp_body<T, C1, C2, CX, false, NW, -1>(a, (int)(s % per), smem);
}

// ------------------------------------------------------------------------------------------
// Data parallelism, FNN_DP_COLLECTIVE_P2P: the update launch that IS the all-reduce.  Every rank's exchange region
// ([2 parities][nbp floats] buckets, then 8 flags on 64-byte lines of their own) is mapped by every peer (hipIpc*).
//   1. block 0, lane p: release at system scope (this rank's bucket of the step -- written by the launch before this one -- is
//      visible to every device), then store the step number into flag[rank] of PEER p's region;
//   2. every block, lane p: poll flag[p] of its OWN region (acquire, system scope) until it holds this step's number -- peer p
//      has published; bounded by the clock (default 30 s, $FNN_P2P_TIMEOUT_MS: a first version counted ~2.5 s of polls, which a peer
//      process that was merely late at start-up could exceed -- met in a two-process rehearsal): a peer that never arrives raises
//      bit 4 of the error word and the block leaves without touching the weights;
//   3. sum the world's buckets in RANK order (every rank forms the same sum, bit for bit) and apply
//      theta <- theta - lr * (sum + L2 term) with the shadow refresh of k_update.
// Reuse of a parity buffer is safe without a second signal: a rank rewrites bucket[n & 1] in step n + 2, after its step n + 1
// launch saw every peer's flag n + 1, which a peer raises only after its own step-n launch (the reader of bucket[n & 1]) ended.
// Flags only grow (64-bit step numbers): nothing is ever reset.
// ------------------------------------------------------------------------------------------
struct P2PArgs {
    float* peer[8]; int world, rank; unsigned long long step; size_t bucket_off, flag_off; int* err;
    unsigned long long timeout_ticks;      // of the constant 100 MHz clock (s_memrealtime): how long a workgroup waits for a peer's flag
    unsigned long long* wait_max;          // the longest wait any step has seen so far (block 0's pollers), same clock: a diagnostic
};

template <typename T>
static __global__ __launch_bounds__(256) void k_p2p_update(const P2PArgs pa, float* __restrict__ master, const float lr, const float lambda1,
                                                    const int reg_all, const int K1p, const int H1p, const int H2p, T* __restrict__ w1,
                                                    T* __restrict__ w1t, T* __restrict__ w2, T* __restrict__ w2t, float* __restrict__ bb0,
                                                    const size_t nw12, const size_t nw, const size_t nbag)
{
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    if (tid == 0) s_bad = 0;
    if (blockIdx.x == 0 && tid < pa.world) {
        unsigned long long* f = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(pa.peer[tid]) + pa.flag_off) + (size_t)pa.rank * 8;
        __hip_atomic_store(f, pa.step, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __syncthreads();
    if (tid < pa.world) {                                       // one wave per workgroup polls (and performs the system-scope acquire)
        const unsigned long long* f = reinterpret_cast<const unsigned long long*>(reinterpret_cast<const char*>(pa.peer[pa.rank]) + pa.flag_off) + (size_t)tid * 8;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < pa.step) {
            if (__builtin_amdgcn_s_memrealtime() - t0 > pa.timeout_ticks) { s_bad = 1; break; }
            __builtin_amdgcn_s_sleep(8);
        }
        if (blockIdx.x == 0) atomicMax(pa.wait_max, __builtin_amdgcn_s_memrealtime() - t0);
    }
    __syncthreads();                                            // the other waves read the buckets behind this barrier
    if (s_bad) { if (tid == 0) atomicOr(pa.err, 16); return; }
    // W1p | W2p: 4 consecutive elements per thread (16-byte bucket reads from every rank, rank order), as in k_step3's dense role
    const size_t nvec = nw12 / 4;
    const int nvb = (int)((nvec + 255) / 256);
    const int b = blockIdx.x;
    if (b < nvb) {
        const size_t q = (size_t)b * 256 + tid;
        if (q >= nvec) return;
        const size_t i = q * 4;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int r = 0; r < pa.world; ++r) {
            const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pa.peer[r] + pa.bucket_off + i));
            g.x += v[0]; g.y += v[1]; g.z += v[2]; g.w += v[3];
        }
        float4 w = *reinterpret_cast<const float4*>(master + i);
        const float l2 = reg_all ? 2.0f * lambda1 : 0.0f;
        w.x -= lr * (g.x + l2 * w.x); w.y -= lr * (g.y + l2 * w.y);
        w.z -= lr * (g.z + l2 * w.z); w.w -= lr * (g.w + l2 * w.w);
        *reinterpret_cast<float4*>(master + i) = w;
        const size_t n1 = (size_t)K1p * H1p;
        const bool first = i < n1;
        const size_t j = first ? i : i - n1;
        const int ld = first ? H1p : H2p, kin = first ? K1p : H1p;
        const int r = (int)(j / ld), c = (int)(j % ld);
        T* wn = first ? w1 : w2;
        T* wt = first ? w1t : w2t;
        store4(wn + ft_off<T>(r, c, ld), w.x, w.y, w.z, w.w);
        wt[ft_off<T>(c, r, kin)] = (T)w.x; wt[ft_off<T>(c + 1, r, kin)] = (T)w.y;
        wt[ft_off<T>(c + 2, r, kin)] = (T)w.z; wt[ft_off<T>(c + 3, r, kin)] = (T)w.w;
        return;
    }
    const size_t i = nw12 + (size_t)(b - nvb) * 256 + tid;      // w3p, then the bag bias: one element each
    if (i >= nw + nbag) return;
    float g = 0.f;
    for (int r = 0; r < pa.world; ++r) g += __builtin_nontemporal_load(pa.peer[r] + pa.bucket_off + i);
    if (i >= nw) { bb0[i - nw] -= lr * g; return; }             // python/SNN_RBM.py:289
    const float w = master[i];
    g += 2.0f * lambda1 * w;                                     // w3, b3 are always regularised (python/FNN_wnzh.py:173)
    master[i] = w - lr * g;
}

}  // namespace fnn
