// ip_group_kernels.hip.h -- the group forms of the inner-product family's kernels (gfx950 only): one launch serves several
// handles, the MODEL as blockIdx.y, every workgroup reading its member's arguments from a device array and running the solo
// kernel's body on them.  A part of the unit ipnn_api.hip, which alone includes it.
//   IpGroupArg   a member's record of ipnn_predict_multi / ipnn_eval_multi: k_ip_fwd_g / _m_g / _w_g and k_ip_strip_fwd_g
//                (ip_launch_class), and k_ip_gflags, the members' range bits (ipnn_eval_multi)
//   IpStepArg    a member's record of ipnn_train_step_multi: every stage of the step, k_mask_draw_g .. k_ip_update_all_g
//                (ip_launch_step_class), and k_ip_step_pack, the results of members that ran their own step
// The records are filled by ip_fill_group_arg / ip_fill_step_arg and reach the device through hs[0]'s rings (arg_ring.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fnn_kernels.hip.h"
#include "sparse_rows.hip.h"
#include "ip_gather_kernels.hip.h"
#include "ip_strip_kernels.hip.h"
#include "ip_step_kernels.hip.h"

namespace {
using namespace fnn;

// ------------------------------------------------------------------------------------------
// Group forms (ipnn_predict_multi / ipnn_eval_multi): the prediction of several handles on one feed batch in two launches with
// the MODEL as blockIdx.y.  A workgroup reads its member's arguments from a device array (IpGroupArg, sent through hs[0]'s
// ArgRing) and runs the solo kernels' bodies on them: blockIdx.x stays the example tile / the strip, so the bodies are the solo
// kernels' own.  The gather writes the F layout of the member's a[0] only (TL = false); the strip launch is the
// one-workgroup-per-strip form over the whole stack (duo.on = 0: a grid of strips x models exceeds the chip, so no workgroup
// may wait for another -- no swap, no flag).  warm = 0: the arguments are not in the kernel argument segment here.
// ------------------------------------------------------------------------------------------
template <typename T> struct IpGroupArg {
    int* err; int model;                                         // the member's error word and its position in the call (k_ip_gflags)
    IpFwdArgs f; IpManyArgs m; IpWideArgs w;                     // the one its row kind takes
    T* a0;                                                       // the member's a[0]: the hand-off between the two launches
    StripFwdArgs<T> s;
};
template <typename T, int NT, bool WV>
static __global__ __launch_bounds__(NT) void k_ip_fwd_g(const IpGroupArg<T>* __restrict__ g)
{
    const IpFwdArgs a = g[blockIdx.y].f;
    ip_fwd_body<T, NT, WV, false>(a, g[blockIdx.y].a0, nullptr, nullptr);
}
template <typename T, bool WV>
static __global__ __launch_bounds__(256) void k_ip_fwd_m_g(const IpGroupArg<T>* __restrict__ g)
{
    const IpManyArgs a = g[blockIdx.y].m;
    ip_fwd_m_body<T, WV, false>(a, g[blockIdx.y].a0, nullptr, nullptr);
}
template <typename T, bool WV>
static __global__ __launch_bounds__(256) void k_ip_fwd_w_g(const IpGroupArg<T>* __restrict__ g)
{
    const IpWideArgs a = g[blockIdx.y].w;
    ip_fwd_w_body<T, WV, false>(a, g[blockIdx.y].a0, nullptr, nullptr);
}
template <typename T, int RT>
static __global__ __launch_bounds__(64 * STRIP_NW) void k_ip_strip_fwd_g(const IpGroupArg<T>* __restrict__ g, const int capA, const int capB)
{
    strip_fwd_body<T, RT, 4, STRIP_NW>(g[blockIdx.y].s, capA, capB);
}
// The range bits (bit 1 of each member's error word) of the n members behind `args` (element stride `elem` bytes: both element
// types share the header) into flags[their position], then cleared.  One workgroup; no handle is listed twice.
static __global__ __launch_bounds__(256) void k_ip_gflags(const char* __restrict__ args, const size_t elem, const int n, int* __restrict__ flags)
{
    for (int i = threadIdx.x; i < n; i += 256) {
        const IpGroupArg<float>* g = reinterpret_cast<const IpGroupArg<float>*>(args + (size_t)i * elem);
        const int f = *g->err & 1;
        flags[g->model] = f;
        if (f) atomicAnd(g->err, ~1);
    }
}

// ------------------------------------------------------------------------------------------
// Group forms of the training step (ipnn_train_step_multi): every stage of the step for the members of one launch class in ONE
// launch, the MODEL as blockIdx.y.  A workgroup reads its member's record (IpStepArg, sent through hs[0]'s step ring) and runs
// the body the solo kernel runs; blockIdx.x stays what it is in the solo launch.  A member whose extent in x is smaller than the
// grid's returns at once.  The strips are the one-workgroup-per-strip form over the whole stack (duo.on = 0, no tail split,
// warm = 0): a group grid holds more workgroups than the chip holds at once, so no workgroup may wait for another.
// ------------------------------------------------------------------------------------------
template <typename T> struct IpStepArg {
    int model; float* pack;                                      // the member's place in the call; its two floats of the packed results (or null)
    int n_mask, n_scat1, n_wg;                                   // the member's own extents in x: mask tiles, level-1 workgroups, weight-gradient tiles
    int drawn;                                                   // 1: md (the library's draw), 0: mt (the caller's masks)
    MaskDrawArgs md; MaskTArgs mt;
    IpFwdArgs f; T* a0; T* a0T; float* emb;                      // the gather with its inner products
    IpManyArgs m;                                                // ... of a many-field member (33 .. 64 fields): the 8-example forward's, and what the 4-example backward reads of them
    StripFwdArgs<T> s; StripBwdArgs<T> sb;                       // the stack, both directions
    IpBwdArgs ib; const float* dz0; float* gxp; float* gb_part;  // the inner products' backward
    IpBArgs bu;                                                  // b
    ScatArgs sa;                                                 // the sparse rows, both levels
    GemmGroupArgs g;                                             // the weight gradients
    IpUpdArgs u;                                                 // the dense update and the loss sum
};
static_assert(sizeof(IpStepArg<float>) == sizeof(IpStepArg<bf16_t>), "one ring element for both element types");

template <typename T>
static __global__ __launch_bounds__(256) void k_mask_draw_g(const IpStepArg<T>* __restrict__ g)
{
    if ((int)blockIdx.x >= g[blockIdx.y].n_mask || !g[blockIdx.y].drawn) return;
    mask_draw_body<const MaskDrawArgs&>(g[blockIdx.y].md);
}
template <typename T>
static __global__ __launch_bounds__(256) void k_mask_T_g(const IpStepArg<T>* __restrict__ g)
{
    if ((int)blockIdx.x >= g[blockIdx.y].n_mask || g[blockIdx.y].drawn) return;
    mask_T_body<const MaskTArgs&>(g[blockIdx.y].mt);
}
template <typename T, int NT, bool WV>
static __global__ __launch_bounds__(NT) void k_ip_fwd_tg(const IpStepArg<T>* __restrict__ g)
{
    const IpFwdArgs a = g[blockIdx.y].f;
    ip_fwd_body<T, NT, WV, true>(a, g[blockIdx.y].a0, g[blockIdx.y].a0T, g[blockIdx.y].emb);
}
template <typename T, bool WV>
static __global__ __launch_bounds__(256) void k_ip_fwd_m_tg(const IpStepArg<T>* __restrict__ g)
{
    const IpManyArgs a = g[blockIdx.y].m;
    ip_fwd_m_body<T, WV, true>(a, g[blockIdx.y].a0, g[blockIdx.y].a0T, g[blockIdx.y].emb);
}
template <typename T, int RT>
static __global__ __launch_bounds__(64 * STRIP_NW) void k_ip_strip_fwd_tg(const IpStepArg<T>* __restrict__ g, const int capA, const int capB)
{
    strip_fwd_body<T, RT, 4, STRIP_NW>(g[blockIdx.y].s, capA, capB);
}
template <typename T, int RT>
static __global__ __launch_bounds__(64 * STRIP_NW) void k_ip_strip_bwd_g(const IpStepArg<T>* __restrict__ g, const int capA, const int capB)
{
    strip_bwd_body<T, RT, 4, STRIP_NW>(g[blockIdx.y].sb, capA, capB);
}
template <typename T, bool WV>
static __global__ __launch_bounds__(256) void k_ip_bwd_g(const IpStepArg<T>* __restrict__ g)
{
    const IpBwdArgs a = g[blockIdx.y].ib;
    const float* __restrict__ dz = g[blockIdx.y].dz0;
    float* __restrict__ gxp = g[blockIdx.y].gxp;
    float* __restrict__ gb_part = g[blockIdx.y].gb_part;
#include "ip_bwd_code.inc.h"
}
template <typename T, bool WV>
static __global__ __launch_bounds__(256) void k_ip_bwd_m_g(const IpStepArg<T>* __restrict__ g)
{
    const IpManyArgs a = g[blockIdx.y].m;
    ip_bwd_m_body<WV>(a, g[blockIdx.y].dz0, g[blockIdx.y].emb, g[blockIdx.y].gxp, g[blockIdx.y].gb_part);
}
// b of the SGD members, one workgroup per member; and every member's owner count at the state the sort leaves its own (0), in
// front of level 1: a grouping class's sort prepares the count of the buffers it is given only.  An Adam / FTRL member's b is
// k_ip_b_update's own launch, one per such member beside its table pass: inlined here, opt_step came out with its moment updates
// unfused where the solo kernel fuses them (v_pk_mul + v_pk_add against v_pk_fma), and b ended one rounding apart.
template <typename T>
static __global__ __launch_bounds__(256) void k_ip_b_update_g(const IpStepArg<T>* __restrict__ g)
{
    const IpBArgs a = g[blockIdx.x].bu;
    int* const oc = g[blockIdx.x].sa.owner_cnt;
    if (threadIdx.x == 0) *oc = 0;
    if (a.opt) return;
    ip_b_update_body(a.b, a.gb_part, a.ngb, a.opt, a.bmv, a.lr, a.beta1, a.beta2, a.eps, a.err);
}
template <typename T>
static __global__ __launch_bounds__(256) void k_ip_scat1_g(const IpStepArg<T>* __restrict__ g)
{
    if ((int)blockIdx.x >= g[blockIdx.y].n_scat1) return;
    const ScatArgs sa = g[blockIdx.y].sa;
    if (sa.form == SCAT1_SLOT) scat1_body(sa, blockIdx.x);
    else if (sa.form == SCAT1_HALF) scat1h_body(sa, blockIdx.x);
    else scat1q_body(sa, blockIdx.x);
}
template <typename T>
static __global__ __launch_bounds__(256) void k_ip_scat2_g(const IpStepArg<T>* __restrict__ g)
{
    __shared__ double s_sum[16][16];
    const ScatArgs sa = g[blockIdx.y].sa;
    if (sa.form2 == SCAT2_WAVE) scat2w_body(sa, blockIdx.x, gridDim.x);
    else scat2_body(sa, blockIdx.x, gridDim.x, s_sum);
}
template <typename T>
static __global__ __launch_bounds__(256) void k_ip_wgrad_g(const IpStepArg<T>* __restrict__ g)
{
    if ((int)blockIdx.x >= g[blockIdx.y].n_wg) return;
    gemm_group_body<T, 4, 4>(g[blockIdx.y].g, (int)blockIdx.x);
}
template <typename T>
static __global__ __launch_bounds__(256) void k_ip_update_all_g(const IpStepArg<T>* __restrict__ g)
{
    const IpUpdArgs& u = g[blockIdx.y].u;
    float* const pack = g[blockIdx.y].pack;
    // with loss_sum_out: the thread that writes the member's loss sum also writes it, and the member's error word behind it (bit 1:
    // an id outside the table; bit 2: a strip pair gave up), into the call's packed results; the word is cleared here, as ipnn_sync
    // clears it after a solo step that returns its loss
#define UPDATE_ALL_DONE(loss) do { if (pack) { int* e_ = const_cast<int*>(u.err); const int f_ = *e_ & 3; pack[0] = (loss); pack[1] = (float)f_; \
                                               if (f_) atomicAnd(e_, ~f_); } } while (0)
#include "ip_update_all_code.inc.h"
#undef UPDATE_ALL_DONE
}
// the loss sums and error words of members that ran their own step inside a group call, into the packed results (one workgroup)
static __global__ __launch_bounds__(256) void k_ip_step_pack(const char* __restrict__ args, const size_t elem, const int n)
{
    for (int i = threadIdx.x; i < n; i += 256) {
        const IpStepArg<float>* g = reinterpret_cast<const IpStepArg<float>*>(args + (size_t)i * elem);
        int* e = const_cast<int*>(g->u.err);
        const int f = *e & 3;
        g->pack[0] = *g->u.loss_sum; g->pack[1] = (float)f;
        if (f) atomicAnd(e, ~f);
    }
}

}  // namespace
