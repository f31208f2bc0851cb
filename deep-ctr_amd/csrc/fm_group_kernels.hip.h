// fm_group_kernels.hip.h -- the group forms of the FM kernels (gfx950 only): one launch serves several handles, every workgroup
// reading its member's arguments from a device array and running the solo kernel's body (fm_kernels.hip.h) on them.  A part of
// the unit fm_api.hip, which alone includes it.
//   EvalArg   a member's record of fm_predict_multi / fm_eval_multi: k_fm_multi / k_fm_wide_multi (one launch per layout class
//             present) and k_fm_eval_flags, the members' range flags
//   StepArg   a member's record of fm_train_step_multi (with StepTail, its bias / loss tail, and StepPack, its loss and range
//             flag for the host): k_fm_step_fwd / k_fm_step_fwd_wide, k_fm_step_scat1 / _scatw1, k_fm_step_scat2_tail / _scatw2_tail
// The records reach the device through hs[0]'s rings (arg_ring.h); the members stand in class order (fm_plan.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fm_kernels.hip.h"

namespace {
using namespace fnn;

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

}  // namespace
