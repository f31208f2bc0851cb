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
// This file is the host half of the unit: the handle, the dispatch ladder, the calls and the C ABI.  The kernels are in
// fm_kernels.hip.h (solo) and fm_group_kernels.hip.h (group forms), fm_online.hip.h (the online schedule); what n_fields and k
// decide about them is the handle's FmPlan (fm_plan.h, free of HIP), computed once in fm_create.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fm_hip.h"
#include "../../include/fnn_hip.h"
#include "sparse_rows.hip.h"
#include "metrics.hip.h"
#include "optim.hip.h"
#include "fm_online.hip.h"
#include "fm_plan.h"
#include "fm_kernels.hip.h"
#include "fm_group_kernels.hip.h"
#include "arg_ring.h"
#include "group_call.h"

using namespace fnn;

namespace {

thread_local std::string g_fm_err;
inline int rup(int x, int m) { return (x + m - 1) / m * m; }
static_assert(FM_SLOT == SLOT, "fm_plan.h's narrow row is the FNN path's slot");

// (the argument arrays of the group calls reach the device through an ArgRing of the handle in front: arg_ring.h)

}  // namespace

// F, K, wide (k >= 17: fm_wide_body, scatw1_body / scatw2_body), rw (the row stride in floats: SLOT for k <= 16, rup(k, 4) on the
// wide path), K1p, and the layout class, fields per lane, examples per workgroup and update form of its kernels: the FmPlan
struct fm_handle : FmPlan {
    std::string err; int dev = 0; hipStream_t st = nullptr; bool own_stream = false;
    int Bmax = 0;
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
// The grouping of a step's batch on handle h as arguments: the run sort (so: launch 1, launch_sort_runs) and its rank-merge
// twin (sb: 16 F workgroups beside the forward, sortB_body), which claims a fresh stamp and marks the rows under several
// columns while fm_set_shared_rows is on -- and only then.
struct StepSort { SortArgs so, sb; };
StepSort step_sort(fm_handle* h, const int32_t* ids, int B)
{
    StepSort s;
    s.so = SortArgs{ids, B, h->F, h->n_rows, h->rg.rec, h->rg.owner_cnt, 4 * h->F, h->skeys};
    s.so.merge4 = h->sort_merge4;
    s.sb = s.so; s.sb.nblk = 16 * h->F;
    if (h->shared) { s.sb.tag_first = h->tag_first; s.sb.tag_shared = h->tag_shared; s.sb.stamp = fm_next_stamp(h); }
    return s;
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

// The dispatch ladder, written once.  A plan's fields per lane (= chunks of 16 fields: NF = NC = ceil(F / 16), 1 up to 16 fields),
// whether the feed carries value weights (without them the kernels are the ones that never read a weight) and the plan's layout
// class reach fn as compile-time constants, fn(Rung<LAY, N, WV>{}); the keyed form adds the width of the sort keys, as a value
// of the key type, where a rank merge rides beside the forward.  The three launch sites -- launch_fwd (the solo forward),
// launch_step_fwd (launch 2 of the step group) and launch_eval_fwd (the evaluation group, beside eval_forward) -- each name their
// own kernel family (its narrow kernel and its wide twin) and nothing else.  The kernel templates come out in the device code in
// the order of their first use, site by site in the order of this file; tools/cmp_kernel_asm.py compares them by symbol, and
// glues what follows a kernel in the plain .text section to it -- so fm_online.hip.h is included in front of the FM kernels'
// headers and launch_eval_fwd stays the last site of the file, as in the commit the comparison was first made against.
template <int LAY, int N, bool WV> struct Rung {
    static constexpr int n = N, lanes = LAY == FM_WIDE32 ? 32 : 16;    // lanes an example on wide rows
    static constexpr bool wide = LAY != FM_NARROW, wv = WV;
};
template <class Fn> void fm_ladder(const FmPlan& p, bool wv, Fn fn)
{
    auto by_layout = [&](auto n, auto w) {
        constexpr int N = decltype(n)::value;
        constexpr bool WV = decltype(w)::value;
        if (p.layout == FM_NARROW) fn(Rung<FM_NARROW, N, WV>{});
        else if (p.layout == FM_WIDE16) fn(Rung<FM_WIDE16, N, WV>{});
        else fn(Rung<FM_WIDE32, N, WV>{});
    };
    auto by_weights = [&](auto n) { if (wv) by_layout(n, std::true_type{}); else by_layout(n, std::false_type{}); };
    switch (p.nf) {
    case 1: by_weights(std::integral_constant<int, 1>{}); break;
    case 2: by_weights(std::integral_constant<int, 2>{}); break;
    case 3: by_weights(std::integral_constant<int, 3>{}); break;
    default: by_weights(std::integral_constant<int, 4>{}); break;
    }
}
template <class Fn> void fm_ladder_keyed(const FmPlan& p, bool wv, bool key64, Fn fn)
{
    fm_ladder(p, wv, [&](auto r) { if (key64) fn(r, (unsigned long long)0); else fn(r, 0u); });
}

// The solo forward on nb workgroups of examples.  sb: the rank merge of the batch's sort runs beside it (training), null: the
// forward alone (predictions).
void launch_fwd(const fm_handle* h, const SortArgs* sb, const FmArgs& a, int nb)
{
    if (!sb) {
        fm_ladder(*h, a.wts != nullptr, [&](auto r) {
            using R = decltype(r);
            if constexpr (!R::wide) hipLaunchKernelGGL((k_fm<R::n, R::wv>), dim3(nb), dim3(256), 0, h->st, a);
            else hipLaunchKernelGGL((k_fm_wide<R::lanes, R::n, R::wv>), dim3(nb), dim3(256), 0, h->st, a);
        });
        return;
    }
    fm_ladder_keyed(*h, a.wts != nullptr, h->key64, [&](auto r, auto key) {
        using R = decltype(r);
        using KT = decltype(key);
        const dim3 grid(sb->nblk + nb);
        if constexpr (!R::wide) hipLaunchKernelGGL((k_fm_merge_fwd<KT, R::n, R::wv>), grid, dim3(256), sort_lds_bytes<KT>(), h->st, *sb, a);
        else hipLaunchKernelGGL((k_fm_wide_merge_fwd<KT, R::lanes, R::n, R::wv>), grid, dim3(256), sort_lds_bytes<KT>(), h->st, *sb, a);
    });
}
// fm_train_step_multi, launch 2 of one layout class (p: the plan of one of its nm members, listed from place `first` on);
// ncls > 0: the rank merges of that many grouping classes in front, mblk workgroups each
void launch_step_fwd(hipStream_t st, const FmPlan& p, bool wv, bool key64, const StepArg* d, int ncls, int mblk, int first, int nm, int tiles)
{
    fm_ladder_keyed(p, wv, key64, [&](auto r, auto key) {
        using R = decltype(r);
        using KT = decltype(key);
        const dim3 grid((unsigned)(ncls * mblk + nm * tiles));
        const size_t lds = ncls ? sort_lds_bytes<KT>() : 0;
        if constexpr (!R::wide) hipLaunchKernelGGL((k_fm_step_fwd<KT, R::n, R::wv>), grid, dim3(256), lds, st, d, ncls, mblk, first, tiles);
        else hipLaunchKernelGGL((k_fm_step_fwd_wide<KT, R::lanes, R::n, R::wv>), grid, dim3(256), lds, st, d, ncls, mblk, first, tiles);
    });
}

// The end of a step, solo or a group member's: Adam's / FTRL's pass over the table (k_fm_opt_pass), or the fold of SGD's lazy
// scale where it is due.
int end_step(fm_handle* h, float lambda, float lr_step)
{
    if (h->opt == FM_OPT_SGD) return fm_fold_due(h->scale) ? fold_scale(h) : FNN_OK;
    const size_t nk = (size_t)h->n_rows * h->K;
    const dim3 grid((unsigned)(((nk + 3) / 4 + 255) / 256));
    if (h->dense_g)
        hipLaunchKernelGGL(k_fm_opt_pass<true>, grid, dim3(256), 0, h->st, h->table16, h->G, h->stamp, (int)h->t, h->s0, h->s1, nk, h->K,
                           h->rw, lambda, h->opt, lr_step, h->beta1, h->beta2, h->eps);
    else
        hipLaunchKernelGGL(k_fm_opt_pass<false>, grid, dim3(256), 0, h->st, h->table16, h->G, h->stamp, (int)h->t, h->s0, h->s1, nk, h->K,
                           h->rw, lambda, h->opt, lr_step, h->beta1, h->beta2, h->eps);
    MHK(h, hipGetLastError());
    return FNN_OK;
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
    launch_fwd(h, nullptr, predict_args(h, ids, wts, B, p_out, fm_wt_env()), (int)fm_tiles(B, h->epb));
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
    const int F = h->F, ex = h->epb, Ba = rup(B, ex);
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
// update; level 2 beside the bias / loss tail; then the end of the step (end_step).
int fm_step(fm_handle* h, const int32_t* ids, const float* wts, const float* y, int B, float lr, float lambda, int reduce_mean, float* p_out)
{
    const StepSort s = step_sort(h, ids, B);
    const bool own_forms = h->form == FM_UPD_NARROW;
    const StepPlan p = plan_step(h, ids, wts, y, B, lr, lambda, reduce_mean, p_out, fm_wt_env(), h, s.sb.stamp,
                                 own_forms ? h->scat_form : SCAT1_HALF, own_forms ? h->scat2_form : SCAT2_WAVE);
    const StepTail& t = p.t;
    launch_sort_runs(h->st, h->key64, s.so);
    launch_fwd(h, &s.sb, p.a, t.n);
#define FM_SCAT(k1, k2_tail) do { \
        hipLaunchKernelGGL(k1, dim3(p.nb1), dim3(256), 0, h->st, p.sa); \
        hipLaunchKernelGGL(k2_tail, dim3(1 + 256), dim3(256), 0, h->st, p.sa, t.b, t.gb_part, t.n, t.lr, t.lambda, t.loss_t, t.Ba, t.lscale, \
                           t.loss_out, t.bo); } while (0)
    if (h->form == FM_UPD_WIDE) FM_SCAT(k_fm_scatw1, k_fm_scatw2_tail);
    else if (h->form == FM_UPD_SHARED) FM_SCAT(k_fm_scat1s, k_fm_scat2s_tail);   // the SHARED forms, with the marks of this step's rank merge
    else FM_SCAT(k_scat1, k_fm_scat2_tail);
#undef FM_SCAT
    MHK(h, hipGetLastError());
    return end_step(h, lambda, p.lr_step);
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
// step_sort() (fm_next_stamp's wrap) and end_step() work on their handle's stream: on_stream() gives them hs[0]'s.
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
    static_cast<FmPlan&>(*h) = fm_make_plan(n_fields, k);
    h->dev = device; h->Bmax = max_batch;
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
        while (n0 + cnt < N && cnt < h->online_chunk && !fold) { s *= dec; ++cnt; fold = fm_fold_due(s); }
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
            for (int m = 0; m < n_models; ++m) { s[m] *= dec[m]; fold = fold || fm_fold_due(s[m]); }
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
            if (fm_fold_due(s[m])) {
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
    const bool key64 = cls[0].lead->key64;
    std::vector<int> order;                                           // classes, the riders first
    for (int c = 0; c < (int)cls.size(); ++c) if (cls[c].lead->key64 == key64) order.push_back(c);
    const int nride = (int)order.size();
    for (int c = 0; c < (int)cls.size(); ++c) if (cls[c].lead->key64 != key64) order.push_back(c);
    std::vector<SortArgs> sorts(cls.size());
    for (int i = 0; i < (int)order.size(); ++i) {
        Cls& k = cls[order[i]];
        fm_handle* h = k.lead;
        const StepSort s = on_stream(h, st, [&] { return step_sort(h, ids, B); });
        launch_sort_runs(st, h->key64, s.so);                         // launch 1
        k.stamp = s.sb.stamp;
        sorts[i] = a[i].so = s.sb;
    }
    MHK(h0, hipGetLastError());

    // plans into the ring, the members listed by forward layout (launch 2) and by update form (launches 3 and 4)
    const bool wt = fm_wt_env();
    std::vector<float> lr_step(M);
    int nb1max[FM_UPDATE_FORMS] = {0, 0, 0};
    for (int m = 0; m < M; ++m) {
        fm_handle* h = hs[m];
        const Cls& k = cls[cls_of[m]];
        const StepPlan p = plan_step(h, ids, wts, y, B, lr[m], lambda[m], reduce_mean ? reduce_mean[m] : 0, p_out ? p_out[m] : nullptr, wt,
                                     k.lead, k.stamp, SCAT1_HALF, SCAT2_WAVE);
        a[m].a = p.a; a[m].sa = p.sa; a[m].t = p.t; a[m].nb1 = p.nb1;
        lr_step[m] = p.lr_step;
        a[m].own_marks = nullptr; a[m].own_stamp = 0;
        if (h->shared && h != k.lead) { a[m].own_marks = h->tag_shared; a[m].own_stamp = on_stream(h, st, [&] { return fm_next_stamp(h); }); }
        a[m].pack = pack ? pack + m : nullptr;
        nb1max[h->form] = std::max(nb1max[h->form], p.nb1);
    }
    const auto fw = members_in_class_order<FM_LAYOUTS>(M, [&](int m) { return hs[m]->layout; }, [&](int j, int m) { a[j].fcls = m; });
    const auto up = members_in_class_order<FM_UPDATE_FORMS>(M, [&](int m) { return hs[m]->form; }, [&](int j, int m) { a[j].scls = m; });
    rc = ring_send(h0, h0->step_ring, slot, (size_t)M);
    if (rc != FNN_OK) return rc;

    for (int i = nride; i < (int)order.size(); ++i) {                 // the other key width: the plain rank merge
        const SortArgs& so = sorts[i];
        if (!key64) hipLaunchKernelGGL((k_sortB<unsigned long long>), dim3(so.nblk), dim3(256), sort_lds_bytes<unsigned long long>(), st, so);
        else hipLaunchKernelGGL((k_sortB<unsigned>), dim3(so.nblk), dim3(256), sort_lds_bytes<unsigned>(), st, so);
    }
    int ride = nride;                                                 // launch 2: the merges ride in the first layout present
    for (int c = 0; c < FM_LAYOUTS; ++c) {
        if (!fw.cnt[c]) continue;
        const FmPlan& pl = *hs[a[fw.first[c]].fcls];                  // a member of the layout
        launch_step_fwd(st, pl, wts != nullptr, key64, d, ride, 16 * F, fw.first[c], fw.cnt[c], (int)fm_tiles(B, pl.epb));
        ride = 0;
    }
    MHK(h0, hipGetLastError());
    using UpdateKernel = void (*)(const StepArg*, int);              // by FmUpdateForm: narrow, narrow shared, wide
    const UpdateKernel level1[FM_UPDATE_FORMS] = {k_fm_step_scat1<false>, k_fm_step_scat1<true>, k_fm_step_scatw1};
    const UpdateKernel level2_tail[FM_UPDATE_FORMS] = {k_fm_step_scat2_tail<false>, k_fm_step_scat2_tail<true>, k_fm_step_scatw2_tail};
    for (int f = 0; f < FM_UPDATE_FORMS; ++f)                         // launch 3
        if (up.cnt[f]) hipLaunchKernelGGL(level1[f], dim3(nb1max[f], up.cnt[f]), dim3(256), 0, st, d, up.first[f]);
    for (int f = 0; f < FM_UPDATE_FORMS; ++f)                         // launch 4
        if (up.cnt[f]) hipLaunchKernelGGL(level2_tail[f], dim3(1 + 256, up.cnt[f]), dim3(256), 0, st, d, up.first[f]);
    MHK(h0, hipGetLastError());
    for (int m = 0; m < M; ++m) {                                     // the end of each member's step
        fm_handle* h = hs[m];
        const int re = on_stream(h, st, [&] { return end_step(h, lambda[m], lr_step[m]); });
        if (re != FNN_OK) return g.member_failed(re, h, m);
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
    h->form = fm_update_form(*h, want);                           // the plan's one entry that is not n_fields' and k's alone
    h->step_stamp = 0;                                           // no step has run under this setting
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

// The forwards of the nm members of one layout class in an evaluation group (eval_forward), from place `first` of the array on;
// p: the plan of one of them.
void launch_eval_fwd(hipStream_t st, const FmPlan& p, bool wv, dim3 grid, const EvalArg* d, int first, int nm, int64_t tiles, int model_fast)
{
    fm_ladder(p, wv, [&](auto r) {
        using R = decltype(r);
        if constexpr (!R::wide) hipLaunchKernelGGL((k_fm_multi<R::n, R::wv>), grid, dim3(256), 0, st, d, first, nm, tiles, model_fast);
        else hipLaunchKernelGGL((k_fm_wide_multi<R::lanes, R::n, R::wv>), grid, dim3(256), 0, st, d, first, nm, tiles, model_fast);
    });
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
    const bool wt = fm_wt_env();
    for (int m = 0; m < g; ++m) a[m].a = predict_args(hs[m], ids, wts, (int)N, p[m], wt);
    const auto lay = members_in_class_order<FM_LAYOUTS>(g, [&](int m) { return hs[m]->layout; }, [&](int j, int m) { a[j].cls = m; });
    const hipStream_t st = h0->st;
    rc = ring_send(h0, h0->eval_ring, slot, (size_t)g);
    if (rc != FNN_OK) return rc;
    const char* order = getenv("FM_EVAL_ORDER");                  // "model": the model is the fast index of the grid; default: the tile
    const int model_fast = order && !strcmp(order, "model");
    for (int c = 0; c < FM_LAYOUTS; ++c) {
        if (!lay.cnt[c]) continue;
        const FmPlan& pl = *hs[a[lay.first[c]].cls];               // a member of the layout
        const int64_t tiles = fm_tiles(N, pl.epb), total = tiles * lay.cnt[c];
        const int64_t gx = total < (1 << 22) ? total : (1 << 22);
        const dim3 grid((unsigned)gx, (unsigned)((total + gx - 1) / gx));
        launch_eval_fwd(st, pl, wts != nullptr, grid, d, lay.first[c], lay.cnt[c], tiles, model_fast);
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
