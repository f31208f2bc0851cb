// fnn_api.hip -- host side of libfnn_hip.so: the C ABI declared in include/fnn_hip.h.
// Replaces the compiled Theano callables `train` / `predict` (python/FNN_wnzh.py:177-183 of
// Atomu2014/deep-ctr) and the Python gather / sparse-update loops around them (:87-96, :299-306).
// gfx950 only; there is no CPU fallback: without a HIP device every entry point fails loudly.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types and prototypes only: the library is opened with dlopen at fnn_dp_init
#include <dlfcn.h>

#include <algorithm>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fnn_hip.h"
#include "fnn_step_kernels.hip.h"
#include "metrics.hip.h"
#include "arg_ring.h"
#include "group_call.h"

using namespace fnn;

namespace {

thread_local std::string g_create_err;

struct ProfSlot { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; double ms = 0; int64_t n = 0; };

inline int rup(int x, int m) { return (x + m - 1) / m * m; }
constexpr int WIDE_XW_MAX = 4096;    // wide FM rows: largest n_fields * rup(k, 4) (16 fields x k = 128: 2048; 39 x k = 101: 4056)

// The A/B knobs of a handle, read from the environment ONCE, by read_knobs at the top of fnn_create: a variable changed while a
// handle lives does nothing to it.  (Read later, where they always were: FNN_DP_PAYLOAD in dp_setup, FNN_P2P_REGION and
// FNN_P2P_TIMEOUT_MS in fnn_dp_p2p_export.)
struct FnnKnobs {
    int wt_stores = 47;         // FNN_WT_STORES (MlpArgs::wt; 0: plain stores): how the strip kernel's training outputs leave
                                // (bit 32: bf16 on FM rows, the transposed activations 16 bytes per lane, written through or plain as bit 1 says)
    int step1_waves = 8;        // FNN_STEP1_WAVES=4: four waves per strip (the 2-byte element types at hidden 300 / 100 run eight)
    bool step1_fixed = true;    // FNN_STEP1_FORM=generic: never the fixed training instance of the strip kernel (step1_sel)
    bool fused = true;          // FNN_NO_FUSE=1: the layer-by-layer kernels instead of the strip kernel
    int role_off = 0;           // FNN_ROLE_OFF, diagnostics only: 1 sort, 2 dense, 4 sparse roles of launches 2 / 3 skipped (make_roles)
    int splitk = 0;             // FNN_SPLITK=2|4|8|16: split-K of the weight-gradient products (0: the plan's choice; bf16 takes 16 as 8: make_plan)
    int scat2_wgs = 256;        // FNN_SCAT2_WGS=16..1024: workgroups walking the multi-chunk segments in launch 3
    int wgrad_form = -1;        // FNN_WGRAD_FORM=direct|lds (-1: the plan's choice, -2: neither word)
    int scat_form = SCAT1_HALF;      // FNN_SCAT1_FORM: the body of level 1 of the sparse-row update (scat1h_body; quarter: scat1q_body, slot: scat1_body)
    int scat2_form = SCAT2_WAVE;     // FNN_SCAT2_FORM: the body of level 2 of the 16-float rows (scat2w_body, a wave per multi-chunk segment; block: scat2_body)
    int sort_merge4 = 1;        // FNN_SORT_RUNS=4 (the default on FM rows): the run sort leaves 4 runs of 1024 keys per field for the rank merge; 16 (bag mode's default): 16 runs of 256
};

// A launchable kernel: what a selector (step1_sel / step2_sel / step3_sel) returns
template <typename... A> struct FnnKernel { void (*fn)(A...) = nullptr; int threads = 0; size_t lds = 0; };
template <typename T> using Step1Kernel = FnnKernel<MlpArgs<T>>;
using Step2Kernel = FnnKernel<SortArgs, WgradArgs, int, int, ScatArgs>;
using Step3Kernel = FnnKernel<SortArgs, TailArgs, ScatArgs>;
template <typename T> using GroupKernel = FnnKernel<const GroupArg<T>*>;      // the launches of fnn_train_step_multi
static_assert(sizeof(GroupArg<float>) == sizeof(GroupArg<bf16_t>) && sizeof(GroupArg<float>) == sizeof(GroupArg<bs16_t>), "one argument ring serves every element type");
template <typename T> using GroupPredKernel = FnnKernel<const GroupPredArg<T>*, int, int64_t, int, int64_t, int64_t, int>;      // the launch of fnn_predict_multi / fnn_eval_multi
static_assert(sizeof(GroupPredArg<float>) == sizeof(GroupPredArg<bf16_t>) && sizeof(GroupPredArg<float>) == sizeof(GroupPredArg<bs16_t>), "one argument ring serves every element type");

// What the configuration and the knobs decide of every call on a handle: made once, by make_plan and plan_step1 in fnn_create.  The
// half that hangs on the width of the sort keys is plan_keys', which fnn_set_table calls again.  What a call adds is its batch
// length and the shadowed features (step_impl).  DESIGN.md section 4, "The step's host side".
struct FnnPlan {
    // shapes
    int F = 0, K = 0, H1 = 0, H2 = 0, xdim = 0, K1p = 0, H1p = 0, H2p = 0;
    int Bmax = 0, ldT = 0, N2max = 0;
    size_t n1 = 0, n2 = 0, nw12 = 0, nw = 0, nslab = 0;
    bool bf16 = false;          // FNN_PREC_BF16: 2-byte elements
    bool split = false;         // FNN_PREC_BF16X3: 4-byte elements (bs16_t), the f32 mode's layouts
    bool bag = false; int rw = SLOT; size_t nbag = 0, off_bag = 0;     // FNN_MODE_BAG: bag rows rw floats wide
    bool wide = false;          // FNN_MODE_FM with k >= 17: FM rows of rw = rup(k, 4) floats, w_0 / ones columns F*rw and F*rw + 1
    // paths
    bool strip_shape = false;   // the strip kernel is built for these padded shapes (strip_shape_ok)
    bool strip_ok = false;      // ... and FNN_NO_FUSE does not turn it off: k_step1 instead of gather / fwd1 / fwd2 / head / bwd1 / gx
    int three_launch_max_B = 0; // the longest batch that trains in the three launches: SORT_N where strip_ok, else none does
    int splitk = 4;             // split-K of the weight-gradient products
    int wgrad_lds = 0;          // the bf16 weight-gradient products stage their operands through LDS (wgrad_tile; f32 and the bf16 pairs keep their register ring)
    // kernels
    FnnKernel<> step1[2];       // [train]: a Step1Kernel<T> of the handle's element type (launch_step1 casts it back)
    bool key64 = false;         // 64-bit sort keys (row << 12 | t does not fit 32 bits)
    Step2Kernel step2[2];       // [the launch carries LDS-form weight gradients]; lds: the sort role's share
    Step3Kernel step3[2];       // [update]
};

}  // namespace

struct fnn_handle : FnnPlan {
    fnn_cfg cfg{};
    std::string err;
    int dev = 0;
    hipStream_t st = nullptr;
    bool own_stream = false;
    FnnKnobs kn;
    std::vector<void*> owned;   // device buffers that live as long as the handle (alloc_owned): fnn_destroy frees them from this record
    float* bb0 = nullptr; void* dlxT = nullptr; void* onesT = nullptr; float* gx_raw = nullptr;     // bag mode
    // FM table
    float* table16 = nullptr; int32_t* field_of_row = nullptr; int64_t n_rows = 0; float w0 = 0.f;
    // dense
    float* master = nullptr; float* bucket = nullptr; float* slab = nullptr;
    void *w1 = nullptr, *w1t = nullptr, *w2 = nullptr, *w2t = nullptr;   // shadows (T)
    bool dense_set[3] = {false, false, false};
    // activations (T) and f32 work buffers
    void *xp = nullptr, *xpT = nullptr, *d1 = nullptr, *d1T = nullptr, *d2 = nullptr, *dl2 = nullptr,
         *dl2T = nullptr, *dl1 = nullptr, *dl1T = nullptr;
    float *gxp = nullptr, *loss_t = nullptr, *loss_dev = nullptr;
    void *d2T = nullptr, *dl3T = nullptr;
    // scatter
    // Grouping results (sorted (row, t) records + level-2 work lists), double-buffered: the slot of
    // the batch being trained and the slot the NEXT batch is grouped into during this step.
    // tag_shared / stamp: bag mode, the rows several columns of the slot's batch hold (SortArgs).  One array per slot: the rank
    // merge of batch n + 1 writes its marks in the same launch in which the update of batch n still reads its own.
    struct SortSlot : RowGroupBufs { int* tag_shared = nullptr; int stamp = 0; };
    int* tag_first = nullptr; int tag_stamp = 0;
    SortSlot slot[2]; int cur = 0;
    const int32_t* sorted_ids = nullptr; int sorted_B = 0;      // what slot[cur] holds (nullptr: nothing)
    const int32_t* next_ids = nullptr; int next_B = 0;          // pending fnn_prefetch_ids request
    void* skeys = nullptr;              // phase-A output of the split sort
    double* cpow_dev = nullptr;
    std::vector<double> cpow_host; double cpow_c = -1.0; int cpow_n = 0;
    int* err_flag = nullptr;
    uint8_t* ones_u8 = nullptr;         // all-ones dropout rows for predict
    // host-pointer staging
    int32_t* st_ids = nullptr; float* st_y = nullptr; uint8_t* st_m1 = nullptr; uint8_t* st_m2 = nullptr;
    float* st_p = nullptr; float* st_x = nullptr;
    // step state
    bool in_step = false, update_pending = false, scatter_pending = false, pend_have_next = false;
    int step_B = 0, pend_Ba = 0;
    int prefetch_hits = 0, prefetch_misses = 0;
    // features shadowed in the gather that the next step's sparse-row update still visits (fnn_set_shadowed)
    int32_t* shadow_dev = nullptr; int n_shadow = 0, shadow_cap = 0;
    // data parallelism (fnn_dp_init / fnn_dp_init_custom)
    bool dp = false, dp_own_comm = false; int dp_rank = 0, dp_world = 1, dp_sparse = FNN_DP_SPARSE_LOCAL;
    fnn_allreduce_fn dp_allreduce = nullptr; fnn_allgather_fn dp_allgather = nullptr; void* dp_ctx = nullptr;
    ncclComm_t comm = nullptr;
    int32_t* xg_ids_send = nullptr; int32_t* xg_ids = nullptr; float* xg_gxp = nullptr;    // EXCHANGE: padded shard ids, gathered ids / gx'
    SortSlot gsl; int gN2 = 0; void* gws = nullptr; size_t gws_bytes = 0;      // grouping of a GLOBAL batch (fnn_step_scatter_global), grown on demand
    int cpow_cap = 0;                   // entries allocated in cpow_dev
    bool step_native_dp = false;        // the step in flight runs its own collective (fnn_train_step after fnn_dp_init)
    // what the dense collective carries and who performs it (fnn_dp_set_payload / fnn_dp_set_collective): handle-wide, never per shard
    int dp_payload = FNN_DP_PAYLOAD_SLABS, dp_collective = FNN_DP_COLLECTIVE_CALLBACK;
    // one-shot all-reduce over peer pointers: this rank's exchange region = [2 parities][xr_nbp floats] buckets, then 8 flags of 64 B
    float* xr = nullptr; size_t xr_nbp = 0, xr_bytes = 0; int xr_kind = 0; bool xr_same_process = false;
    float* peer[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; bool peer_opened[8] = {false, false, false, false, false, false, false, false};
    bool p2p_attached = false; unsigned long long dp_step_no = 0;
    unsigned long long p2p_timeout_ticks = 3000000000ull;      // 30 s of the 100 MHz clock ($FNN_P2P_TIMEOUT_MS)
    unsigned long long* p2p_wait_max = nullptr;                // device word: the longest flag wait so far (diagnostic)
    int step_bsize = 0;                 // its b_size (the decay table is rebuilt with it when a global batch outgrows the table)
    // fnn_train_step_multi, used when this handle is hs[0]: the argument ring (four calls of the largest group), the event that
    // joins the other members' streams to this one's and back, the packed {loss, range flag} of a call that asks for the losses
    ArgRing step_ring{sizeof(GroupArg<float>), 4 * FNN_STEP_MAX_MODELS};
    hipEvent_t join = nullptr; GroupPack* step_pack = nullptr;
    // fnn_predict_multi / fnn_eval_multi, used when this handle is hs[0]: their argument ring and the zeroed labels of one feed
    // batch that the strip kernel reads (and does not use) while it predicts
    ArgRing eval_ring{sizeof(GroupPredArg<float>), 4 * FNN_EVAL_MAX_MODELS};
    float* eval_y = nullptr;
    // profiling
    bool prof = false;
    std::map<std::string, ProfSlot> prof_slots;
};

// The early returns of every entry point; what follows the named arguments is a cleanup statement run before the return.
// HIPCHK: a failing HIP call leaves "<its text>: <the error's string>"; FAIL: a refusal with its message; RCCHK: a callee's code (and message) passed on.
#define HIPCHK(h, expr, ...) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_); __VA_ARGS__; return FNN_ERR_HIP; } } while (0)
#define FAIL(h, code, msg, ...) do { (h)->err = (msg); __VA_ARGS__; return (code); } while (0)
#define RCCHK(expr, ...) do { const int rc_ = (expr); if (rc_ != FNN_OK) { __VA_ARGS__; return rc_; } } while (0)

namespace {

struct ProfScope {
    fnn_handle* h; hipStream_t s; hipEvent_t b = nullptr, e = nullptr; const char* name;
    ProfScope(fnn_handle* h_, const char* n, hipStream_t s_) : h(h_), s(s_), name(n) {
        if (!h->prof) return;
        hipEventCreate(&b); hipEventCreate(&e); hipEventRecord(b, s);
    }
    ~ProfScope() {
        if (!h->prof) return;
        hipEventRecord(e, s);
        h->prof_slots[name].ev.emplace_back(b, e);
    }
};

template <typename T> int alloc_dev(fnn_handle* h, T** p, size_t n, bool zero = true) {
    HIPCHK(h, hipMalloc((void**)p, n * sizeof(T)));
    if (zero) HIPCHK(h, hipMemsetAsync(*p, 0, n * sizeof(T), h->st));
    return FNN_OK;
}
// a buffer that fnn_create allocates and nothing regrows: recorded as it is allocated, freed by fnn_destroy from the record
template <typename T> int alloc_owned(fnn_handle* h, T** p, size_t n, bool zero = true) {
    const int rc = alloc_dev(h, p, n, zero);
    if (*p) h->owned.push_back(*p);
    return rc;
}

// Host pointers (FNN_MEM_HOST) of a call go through the handle's staging buffers; device pointers pass untouched.  in(): copy an
// input up and point at the copy; out(): point a result at its staging buffer; copy_back(): enqueue the results' way home (the
// caller synchronises).
struct Staged {
    fnn_handle* h; bool host; struct { void* dst; const void* src; size_t bytes; } back[2] = {}; int nback = 0;
    template <typename T> int in(const T*& p, T* buf, size_t n) {
        if (!host) return FNN_OK;
        HIPCHK(h, hipMemcpyAsync(buf, p, n * sizeof(T), hipMemcpyHostToDevice, h->st));
        p = buf;
        return FNN_OK;
    }
    template <typename T> void out(T*& p, T* buf, size_t n) { if (host && p) { back[nback++] = {p, buf, n * sizeof(T)}; p = buf; } }
    int copy_back() {
        for (int i = 0; i < nback; ++i) HIPCHK(h, hipMemcpyAsync(back[i].dst, back[i].src, back[i].bytes, hipMemcpyDeviceToHost, h->st));
        return FNN_OK;
    }
};

size_t tsize(const fnn_handle* h) { return h->bf16 ? 2 : 4; }
// the element type of the handle's precision: FN<T> ARGS
#define BY_PREC(h, FN, ARGS) do { if ((h)->bf16) FN<bf16_t> ARGS; else if ((h)->split) FN<bs16_t> ARGS; else FN<float> ARGS; } while (0)
#define BY_PREC_RC(h, FN, ARGS) ((h)->bf16 ? FN<bf16_t> ARGS : ((h)->split ? FN<bs16_t> ARGS : FN<float> ARGS))

int check_async(fnn_handle* h) {
    int flag = 0;
    HIPCHK(h, hipMemcpyAsync(&flag, h->err_flag, sizeof(int), hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    if (flag) {
        HIPCHK(h, hipMemsetAsync(h->err_flag, 0, sizeof(int), h->st));
        if (flag & 16) FAIL(h, FNN_ERR_HIP, "data-parallel p2p all-reduce: a peer's flag did not arrive in time; the dense tensors of that step were left untouched");
        FAIL(h, FNN_ERR_RANGE, "feature id outside [-1, n_rows) (reference: KeyError, python/FNN_wnzh.py:95)");
    }
    return FNN_OK;
}

int update_cpow(fnn_handle* h, int b_size, int B) {
    const double c = 1.0 - 2.0 * (double)h->cfg.lambda_fm * (double)h->cfg.lr / (double)b_size;
    if (c == h->cpow_c && h->cpow_n >= B + 1) return FNN_OK;
    // in-flight kernels may still read the old table
    HIPCHK(h, hipStreamSynchronize(h->st));
    const int n = h->cpow_cap;
    h->cpow_host.resize(n);
    for (int i = 0; i < n; ++i) h->cpow_host[i] = std::pow(c, (double)i);
    HIPCHK(h, hipMemcpy(h->cpow_dev, h->cpow_host.data(), n * sizeof(double), hipMemcpyHostToDevice));
    h->cpow_c = c; h->cpow_n = n;
    return FNN_OK;
}

template <typename T, int NT, typename Epi>
void launch_gemm(hipStream_t s, const T* A, int lda, const T* Bft, int M, int N, int klen, Epi epi) {
    dim3 grid(M / 64, N / (16 * NT), 1);
    hipLaunchKernelGGL((k_gemm<T, NT, Epi>), grid, dim3(256), 0, s, A, lda, Bft, klen, epi);
}

// refresh shadows from the masters without a gradient step
template <typename T> void launch_update(fnn_handle* h, const float* bucket, float lr) {
    const size_t n = h->nw;
    hipLaunchKernelGGL((k_update<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->master,
                       bucket, lr, h->cfg.lambda1, h->cfg.reg_all, h->K1p, h->H1p, h->H2p, (T*)h->w1, (T*)h->w1t,
                       (T*)h->w2, (T*)h->w2t);
    if (h->bag && bucket)
        hipLaunchKernelGGL(k_axpy, dim3((unsigned)((h->nbag + 255) / 256)), dim3(256), 0, h->st, h->bb0,
                           bucket + h->nw, -lr, (int)h->nbag);
}

// the strip kernel is instantiated for the padded shapes in use; anything else takes the
// layer-by-layer kernels
bool strip_shape_ok(const FnnPlan& p) {
    if (p.wide) return false;                                // the strip kernel reads 16-float slots
    const int c1 = p.H1p / 64, c2 = p.H2p / 64, cx = p.K1p / 64;
    if (cx == 5) return p.bag && c1 == 5 && c2 == 2;         // bag rows 256..316 wide: the reference's default hidden0 = 300 (python/SNN_RBM.py:25)
    return cx == 4 && ((c1 == 5 && c2 == 2) || (c1 == 1 && c2 == 1));
}
// a fresh stamp for a grouping about to be written into `sl` (bag mode; see SortArgs).  2^25 groupings, then the tags start over.
int next_stamp(fnn_handle* h, fnn_handle::SortSlot& sl) {
    if (!h->bag) return 0;
    if (h->tag_stamp >= (1 << 25) - 1) {
        hipMemsetAsync(h->tag_first, 0, (size_t)h->n_rows * sizeof(int), h->st);
        for (auto& q : h->slot) hipMemsetAsync(q.tag_shared, 0, (size_t)h->n_rows * sizeof(int), h->st);
        h->tag_stamp = 0;
    }
    sl.stamp = ++h->tag_stamp;
    return sl.stamp;
}
int sort_n2(int B) { int N2 = 256; while (N2 < B) N2 <<= 1; return N2; }
constexpr int GLOBAL_BATCH_MAX = 32768;        // fnn_step_scatter_global / FNN_DP_SPARSE_EXCHANGE: 8 ranks x 4096 examples

template <typename T> WgradArgs make_wgrad_args(fnn_handle* h, int Ba) {
    WgradArgs wa;
    wa.p[0] = WgradProb{h->xpT, h->dl1T, h->slab, h->K1p / 64, h->H1p / 64, h->H1p};
    wa.p[1] = WgradProb{h->d1T, h->dl2T, h->slab + h->n1, h->H1p / 64, h->H2p / 64, h->H2p};
    wa.p[2] = WgradProb{h->d2T, h->dl3T, h->slab + h->nw12, h->H2p / 64, 1, 64};     // gw3p = column 0
    wa.p[3] = WgradProb{h->dlxT, h->onesT, h->slab + h->off_bag, h->bag ? h->K1p / 64 : 0, 1, 64};   // sum_t delta_t
    wa.ldT = h->ldT; wa.klen = Ba / h->splitk; wa.zstride = h->nslab;
    return wa;
}
int wgrad_blocks(const WgradArgs& wa) {
    return wa.p[0].mt * wa.p[0].nt + wa.p[1].mt * wa.p[1].nt + wa.p[2].mt * wa.p[2].nt + wa.p[3].mt * wa.p[3].nt;
}
ScatArgs make_scat_args(fnn_handle* h, const fnn_handle::SortSlot& sl, int N2) {
    ScatArgs sa = scat_args(sl, N2, h->F, h->K, h->gxp, h->K1p, h->cpow_dev, (double)h->cfg.lr, h->table16, h->rw);
    sa.tag_shared = sl.tag_shared; sa.stamp = sl.stamp; sa.form2 = h->kn.scat2_form;
    return sa;
}
template <typename T> MlpArgs<T> make_mlp_args(fnn_handle* h, const int32_t* ids, const float* y, int B,
                                                const uint8_t* m1, const uint8_t* m2, bool train, float* p_out) {
    return MlpArgs<T>{ids, y ? y : h->loss_t, B, h->F, h->K, h->table16, h->n_rows, h->w0,
                      (const T*)h->w1, (const T*)h->w1t, (const T*)h->w2, (const T*)h->w2t, h->master + h->nw12,
                      m1 ? m1 : h->ones_u8, m2 ? m2 : h->ones_u8, h->cfg.act, train ? ACT_TANH : h->cfg.act,
                      h->H1, h->H2, train ? 1 : 0,
                      (T*)h->xpT, (T*)h->d1T, (T*)h->d2T, (T*)h->dl1T, (T*)h->dl2T, (T*)h->dl3T, h->ldT,
                      h->gxp, p_out, h->loss_t, h->err_flag, h->bb0, h->rw, (T*)h->dlxT, nullptr, h->kn.wt_stores};
}
// ---- kernel selectors: the only places that name an instantiation of k_step1, k_step2 or k_step3
// The strip kernel by padded shape (strip_shape_ok), waves per strip and form.  Hidden 300 / 100 runs EIGHT waves per strip (two
// per SIMD), a layer's 16-column fragments in runs of ceil(n / 8) per wave -- the strip is a chain of phases, each as long as its
// busiest wave's run (FNN_STEP1_WAVES=4: four waves).  The fixed training form (mlp_body, WTF): a training step of the default
// store policy in bf16 on FM rows, whose gather is one trip of the workgroup (8-example pieces in groups of 16, two lanes each:
// F <= 32); FNN_STEP1_FORM=generic and everything else -- prediction, any other FNN_WT_STORES -- run the instance that reads its flags.
template <typename T> Step1Kernel<T> step1_sel(const FnnPlan& p, const FnnKnobs& kn, bool train)
{
#define STEP1(C1, C2, CX, BAG, NW, ...) Step1Kernel<T>{k_step1<T, C1, C2, CX, BAG, NW, ##__VA_ARGS__>, 64 * NW, mlp_lds_bytes<T, C1, C2, CX>(BAG, p.F, NW)}
    const bool big = p.H1p / 64 == 5, x5 = p.K1p / 64 == 5;             // x5: bag mode only (strip_shape_ok)
    if (big && kn.step1_waves == 8) {
        if (x5) return STEP1(5, 2, 5, true, 8);
        if (p.bag) return STEP1(5, 2, 4, true, 8);
        if constexpr (std::is_same<T, bf16_t>::value)
            if (kn.step1_fixed && train && kn.wt_stores == 47 && ((8 * p.F + 15) >> 4) * 32 <= 512) return STEP1(5, 2, 4, false, 8, 47);
        return STEP1(5, 2, 4, false, 8);
    }
    if (x5) return STEP1(5, 2, 5, true, 4);
    if (p.bag) return big ? STEP1(5, 2, 4, true, 4) : STEP1(1, 1, 4, true, 4);
    return big ? STEP1(5, 2, 4, false, 4) : STEP1(1, 1, 4, false, 4);
#undef STEP1
}
// launch 2 by key width x merge form x weight-gradient form (the LDS form: 2-byte elements only); lds: the run sort's share
template <typename T> Step2Kernel step2_sel(bool key64, bool m4, bool wgrad_lds)
{
#define STEP2(WF) (key64 ? (m4 ? Step2Kernel{k_step2<T, unsigned long long, true, WF>, 256, lds} : Step2Kernel{k_step2<T, unsigned long long, false, WF>, 256, lds}) \
                         : (m4 ? Step2Kernel{k_step2<T, unsigned, true, WF>, 256, lds} : Step2Kernel{k_step2<T, unsigned, false, WF>, 256, lds}))
    const size_t lds = key64 ? sortA_lds_bytes<unsigned long long>(m4) : sortA_lds_bytes<unsigned>(m4);
    if constexpr (sizeof(T) == 2) if (wgrad_lds) return STEP2(WGRAD_LDS);
    return STEP2(WGRAD_DIRECT);
#undef STEP2
}
// launch 3 by key width x merge form x update; lds: the rank merge's
template <typename T> Step3Kernel step3_sel(bool key64, bool m4, bool update)
{
#define STEP3(KT, LDS) (m4 ? (update ? Step3Kernel{k_step3<T, true, KT, true>, 256, LDS} : Step3Kernel{k_step3<T, false, KT, true>, 256, LDS}) \
                           : (update ? Step3Kernel{k_step3<T, true, KT, false>, 256, LDS} : Step3Kernel{k_step3<T, false, KT, false>, 256, LDS}))
    return key64 ? STEP3(unsigned long long, sort_lds_bytes<unsigned long long>()) : STEP3(unsigned, sort_lds_bytes<unsigned>());
#undef STEP3
}
// ---- the group kernels of fnn_train_step_multi: the training forms on FM rows that step1_sel(train = true), step2_sel and
// step3_sel(update = true) can return, chosen by the same conditions; the only places that name an instantiation of k_gstep*
template <typename T> GroupKernel<T> gstep1_sel(const FnnPlan& p, const FnnKnobs& kn)
{
#define GSTEP1(C1, C2, NW, WTF) GroupKernel<T>{k_gstep1<T, C1, C2, 4, NW, WTF>, 64 * NW, mlp_lds_bytes<T, C1, C2, 4>(false, p.F, NW)}
    const bool big = p.H1p / 64 == 5;
    if (big && kn.step1_waves == 8) {
        if constexpr (std::is_same<T, bf16_t>::value)
            if (kn.step1_fixed && kn.wt_stores == 47 && ((8 * p.F + 15) >> 4) * 32 <= 512) return GSTEP1(5, 2, 8, 47);
        return GSTEP1(5, 2, 8, -1);
    }
    return big ? GSTEP1(5, 2, 4, -1) : GSTEP1(1, 1, 4, -1);
#undef GSTEP1
}
// ... and of fnn_bag_train_step_multi: the strips of bag rows, the instances that step1_sel(train = true) returns for a bag handle
template <typename T> GroupKernel<T> gstep1_bag_sel(const FnnPlan& p, const FnnKnobs& kn)
{
#define GSTEP1B(C1, C2, CX, NW) GroupKernel<T>{k_gstep1<T, C1, C2, CX, NW, -1, true>, 64 * NW, mlp_lds_bytes<T, C1, C2, CX>(true, p.F, NW)}
    const bool big = p.H1p / 64 == 5, x5 = p.K1p / 64 == 5;
    if (big && kn.step1_waves == 8) return x5 ? GSTEP1B(5, 2, 5, 8) : GSTEP1B(5, 2, 4, 8);
    if (x5) return GSTEP1B(5, 2, 5, 4);
    return big ? GSTEP1B(5, 2, 4, 4) : GSTEP1B(1, 1, 4, 4);
#undef GSTEP1B
}
// ---- the group kernel of fnn_predict_multi / fnn_eval_multi: the generic instance on FM rows that step1_sel(train = false)
// returns, by the same conditions; the only place that names an instantiation of k_gpredict
template <typename T> GroupPredKernel<T> gpredict_sel(const FnnPlan& p, const FnnKnobs& kn)
{
#define GPREDICT(C1, C2, NW) GroupPredKernel<T>{k_gpredict<T, C1, C2, 4, NW>, 64 * NW, mlp_lds_bytes<T, C1, C2, 4>(false, p.F, NW)}
    const bool big = p.H1p / 64 == 5;
    if (big && kn.step1_waves == 8) return GPREDICT(5, 2, 8);
    return big ? GPREDICT(5, 2, 4) : GPREDICT(1, 1, 4);
#undef GPREDICT
}
template <typename T> GroupKernel<T> gstep2_sel(bool key64, bool m4, bool wgrad_lds)
{
#define GSTEP2(WF) (key64 ? (m4 ? GroupKernel<T>{k_gstep2<T, unsigned long long, true, WF>, 256, lds} : GroupKernel<T>{k_gstep2<T, unsigned long long, false, WF>, 256, lds}) \
                          : (m4 ? GroupKernel<T>{k_gstep2<T, unsigned, true, WF>, 256, lds} : GroupKernel<T>{k_gstep2<T, unsigned, false, WF>, 256, lds}))
    const size_t lds = key64 ? sortA_lds_bytes<unsigned long long>(m4) : sortA_lds_bytes<unsigned>(m4);
    if constexpr (sizeof(T) == 2) if (wgrad_lds) return GSTEP2(WGRAD_LDS);
    return GSTEP2(WGRAD_DIRECT);
#undef GSTEP2
}
template <typename T> GroupKernel<T> gstep3_sel(bool key64, bool m4)
{
#define GSTEP3(KT) (m4 ? GroupKernel<T>{k_gstep3<T, KT, true>, 256, sort_lds_bytes<KT>()} : GroupKernel<T>{k_gstep3<T, KT, false>, 256, sort_lds_bytes<KT>()})
    return key64 ? GSTEP3(unsigned long long) : GSTEP3(unsigned);
#undef GSTEP3
}
// the plan's kernels: launch 1 for prediction and training, made at create ...
template <typename T> void plan_step1(fnn_handle* h)
{
    for (int train = 0; train < 2; ++train) {
        const Step1Kernel<T> k = step1_sel<T>(*h, h->kn, train != 0);
        h->step1[train] = {reinterpret_cast<void (*)()>(k.fn), k.threads, k.lds};
    }
}
// ... and launches 2 and 3, which change with the width of the sort keys: at create and whenever a table is set
template <typename T> void plan_keys(fnn_handle* h, bool key64)
{
    h->key64 = key64;
    for (int i = 0; i < 2; ++i) {
        h->step2[i] = step2_sel<T>(key64, h->kn.sort_merge4 != 0, i && h->wgrad_lds);
        h->step3[i] = step3_sel<T>(key64, h->kn.sort_merge4 != 0, i != 0);
    }
}

template <typename T> void launch_step1(fnn_handle* h, int nmlp, const MlpArgs<T>& a) {
    const FnnKernel<>& k = h->step1[a.train];
    hipLaunchKernelGGL(reinterpret_cast<void (*)(MlpArgs<T>)>(k.fn), dim3(nmlp), dim3(k.threads), k.lds, h->st, a);
}
void launch_sort16(fnn_handle* h, SortArgs so) {             // split sort: the runs, then the rank merge
    so.merge4 = h->kn.sort_merge4;
    launch_sort(h->st, h->key64, so);
}

// Launches 2 and 3 of a step, always issued as a pair, and what the pair does.  `dense`: weight gradients / slab reduce (+ `update`,
// into `bucket_dst` if given, else the handle's bucket); `sparse`: the sparse-row SGD of this batch (reading `gxp_src` if given: another
// shard's gathered gradients, bag EXCHANGE) with `group_next`, the grouping of the next one.  Single-GPU and native data-parallel steps
// run both halves in the same two launches (the data-parallel one with its collective between or behind them); the portable split API
// (fnn_step_begin / _scatter / _end) runs the halves separately.
struct StepRoles { bool dense, sparse, group_next, update; const float* gxp_src; float* bucket_dst; };
StepRoles make_roles(const fnn_handle* h, bool dense, bool sparse, bool update, const float* gxp_src = nullptr, float* bucket_dst = nullptr)
{
    const int off = h->kn.role_off;                          // timing experiments: results are wrong by construction
    return {dense && !(off & 2), sparse && !(off & 4), sparse && !(off & 1), update, gxp_src, bucket_dst};
}
// What both launches take: the row update's arguments on the current slot, and the grouping of the next batch into the other one.
// The launches differ in so.nblk (2: four run sorts per field, 3: sixteen rank merges) and in the tag fields, which only the rank
// merge of launch 3 writes (it draws the next slot's stamp, once).
struct Step23Args { bool have_next; ScatArgs sa; SortArgs so; };
Step23Args make_step23_args(fnn_handle* h, const StepRoles& r, bool merge)
{
    const bool have_next = r.group_next && h->pend_have_next;
    fnn_handle::SortSlot& nx = h->slot[h->cur ^ 1];
    Step23Args a{have_next, make_scat_args(h, h->slot[h->cur], SORT_N), {}};
    if (r.gxp_src) a.sa.gxp = r.gxp_src;
    a.so = SortArgs{h->next_ids, h->next_B, h->F, h->n_rows, nx.rec, nx.owner_cnt, have_next ? (merge ? 16 : 4) * h->F : 0, h->skeys,
                    merge ? h->tag_first : nullptr, merge ? nx.tag_shared : nullptr, merge && have_next ? next_stamp(h, nx) : 0, h->kn.sort_merge4};
    return a;
}
const char* role_name(const StepRoles& r, const char* both, const char* dense, const char* sparse) { return r.dense && r.sparse ? both : (r.dense ? dense : sparse); }

template <typename T> void launch_step2(fnn_handle* h, const StepRoles& r)
{
    Step23Args a = make_step23_args(h, r, false);
    ProfScope ps(h, role_name(r, "step2", "step2_dense", "step2_sparse"), h->st);
    const WgradArgs wa = make_wgrad_args<T>(h, h->pend_Ba);
    const int nwx = r.dense ? wgrad_blocks(wa) : 0;
    const int nsc = !r.sparse ? 0 : (h->bag ? (int)(((size_t)h->F * (SORT_N / WCH) * (h->rw / 4) + 255) / 256)
                                            : scat1_blocks(a.sa, h->kn.scat_form));
    const dim3 grid(a.so.nblk + nwx * h->splitk + nsc);
    if (grid.x == 0) return;
    // the LDS form of the weight gradients sizes the launch's dynamic LDS for every role's workgroups
    const bool wl = nwx > 0 && h->wgrad_lds && sizeof(T) == 2;
    const Step2Kernel& k = h->step2[wl];
    hipLaunchKernelGGL(k.fn, grid, dim3(k.threads), std::max(k.lds, wl ? WGRAD_LDS_BYTES : (size_t)0), h->st, a.so, wa, nwx, h->splitk, a.sa);
}

// the dense role of launch 3: its arguments and (nblk_red) its workgroups
TailArgs make_tail_args(const fnn_handle* h, const StepRoles& r)
{
    const int nred = r.dense ? (int)((h->nw12 / 4 + 255) / 256) + (int)((h->nw - h->nw12 + h->nbag + 255) / 256) + 1 : 0;
    return TailArgs{h->slab, h->splitk, h->nw, h->nw12, h->nslab, h->master, h->cfg.lambda1, h->cfg.reg_all,
                    h->loss_t, h->pend_Ba, r.bucket_dst ? r.bucket_dst : h->bucket, h->loss_dev, h->cfg.lr, h->K1p, h->H1p, h->H2p,
                    h->w1, h->w1t, h->w2, h->w2t, nred, h->bb0, h->nbag, h->off_bag};
}
// the sparse role's bookkeeping behind launch 3: the slots flip, nothing is left to scatter
void sparse_role_done(fnn_handle* h, bool have_next)
{
    if (have_next) { h->cur ^= 1; h->sorted_ids = h->next_ids; h->sorted_B = h->next_B; }
    else { h->sorted_ids = nullptr; h->sorted_B = 0; }
    h->next_ids = nullptr; h->next_B = 0;
    h->scatter_pending = false;
}

template <typename T> void launch_step3(fnn_handle* h, const StepRoles& r)
{
    const Step23Args a = make_step23_args(h, r, true);
    {
        ProfScope ps(h, role_name(r, "step3", "step3_dense", "step3_sparse"), h->st);
        const TailArgs ta = make_tail_args(h, r);
        const int nred = ta.nblk_red;
        const dim3 grid(a.so.nblk + nred + (r.sparse ? h->kn.scat2_wgs : 0));    // these workgroups walk the multi-chunk segments
        const Step3Kernel& k = h->step3[r.update];
        if (grid.x > 0) hipLaunchKernelGGL(k.fn, grid, dim3(k.threads), k.lds, h->st, a.so, ta, a.sa);
    }
    if (r.sparse) sparse_role_done(h, a.have_next);
}
template <typename T> void launch_steps23(fnn_handle* h, const StepRoles& r) { launch_step2<T>(h, r); launch_step3<T>(h, r); }

// ---- collectives of the native data-parallel step, enqueued on the handle's stream
int dp_allreduce(fnn_handle* h, float* buf, size_t n, const char* what)
{
    ProfScope ps(h, "allreduce", h->st);
    h->err.clear();                              // the RCCL callback leaves its message here; a caller's callback leaves nothing
    const int rc = h->dp_allreduce(h->dp_ctx, buf, (int64_t)n, (void*)h->st);
    if (rc != 0) FAIL(h, FNN_ERR_HIP, std::string("data-parallel all-reduce (") + what + ") failed" + (h->err.empty() ? std::string(": the callback returned ") + std::to_string(rc) : ": " + h->err));
    return FNN_OK;
}

// Bucket payload: the flat bucket holds THIS rank's dense gradients (launch 3 without its update, or the layer-by-layer
// k_reduce); sum it over the ranks and apply theta <- theta - lr * (sum + L2 term).  Callback collective: all-reduce in place,
// then k_update.  P2P: the bucket sits in (or is copied into) this rank's exchange region and ONE launch does the rest.
inline float* p2p_bucket(fnn_handle* h) { return h->xr + (size_t)(h->dp_step_no & 1) * h->xr_nbp; }
template <typename T> int dp_finish_bucket(fnn_handle* h, bool in_region)
{
    if (h->dp_collective == FNN_DP_COLLECTIVE_P2P) {
        if (!in_region)
            HIPCHK(h, hipMemcpyAsync(p2p_bucket(h), h->bucket, (h->nw + h->nbag) * sizeof(float), hipMemcpyDeviceToDevice, h->st));
        ProfScope ps(h, "p2p_update", h->st);
        P2PArgs pa;
        for (int r = 0; r < 8; ++r) pa.peer[r] = h->peer[r];
        pa.world = h->dp_world; pa.rank = h->dp_rank; pa.step = h->dp_step_no + 1;
        pa.bucket_off = (size_t)(h->dp_step_no & 1) * h->xr_nbp; pa.flag_off = 2 * h->xr_nbp * sizeof(float); pa.err = h->err_flag;
        pa.timeout_ticks = h->p2p_timeout_ticks; pa.wait_max = h->p2p_wait_max;
        const unsigned nblk = (unsigned)((h->nw12 / 4 + 255) / 256 + (h->nw - h->nw12 + h->nbag + 255) / 256);
        hipLaunchKernelGGL((k_p2p_update<T>), dim3(nblk), dim3(256), 0, h->st, pa, h->master, h->cfg.lr,
                           h->cfg.lambda1, h->cfg.reg_all, h->K1p, h->H1p, h->H2p, (T*)h->w1, (T*)h->w1t, (T*)h->w2, (T*)h->w2t,
                           h->bb0, h->nw12, h->nw, h->nbag);
        h->dp_step_no++;
        return FNN_OK;
    }
    RCCHK(dp_allreduce(h, h->bucket, h->nw + h->nbag, "dense-gradient bucket"));
    ProfScope ps(h, "update", h->st);
    launch_update<T>(h, h->bucket, h->cfg.lr);
    return FNN_OK;
}
inline bool dp_bucket_mode(const fnn_handle* h) { return h->dp_collective == FNN_DP_COLLECTIVE_P2P || h->dp_payload == FNN_DP_PAYLOAD_BUCKET; }

int ensure_global_ws(fnn_handle* h, int B_g);
int scatter_global_impl(fnn_handle* h, const int32_t* ids_g, const float* gxp_g, int B_g);

// EXCHANGE: all-gather (ids, gx') of every shard, each padded to ldT rows (empty ids), then the sparse-row SGD of the whole
// global batch in global example order on this rank.
// Bag mode (python/SNN_RBM.py:285-291: ww0[f] -= delta_t, no decay -- a plain sum over the examples): the gathered shards are
// applied ONE AFTER THE OTHER in rank order with the step's own sparse role (grouping of the shard's ids, then the two levels of
// the segmented row update reading that shard's gathered deltas): every rank launches the same operations in the same order, so
// the replicas equal the single-process step of the global batch up to the rounding of `world` partial sums per row instead of
// one, and stay bit-identical to each other while no row sits in two columns of a shard; rows that do take the float atomics of
// the row update, whose order no launch fixes (include/fnn_hip.h).
template <typename T>
int dp_exchange_sparse(fnn_handle* h, const int32_t* ids, int B)
{
    const int rows = h->ldT, F = h->F;
    {
        ProfScope ps(h, "allgather", h->st);
        const size_t n = (size_t)rows * F;
        hipLaunchKernelGGL(k_pad_ids, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, ids, B, F, rows, h->xg_ids_send);
        int rc = h->dp_allgather(h->dp_ctx, h->xg_ids_send, h->xg_ids, (int64_t)(n * 4), (void*)h->st);
        if (rc == 0) rc = h->dp_allgather(h->dp_ctx, h->gxp, h->xg_gxp, (int64_t)((size_t)rows * h->K1p * 4), (void*)h->st);
        if (rc != 0) FAIL(h, FNN_ERR_HIP, "data-parallel all-gather failed: " + h->err);
    }
    if (!h->bag) return scatter_global_impl(h, h->xg_ids, h->xg_gxp, rows * h->dp_world);
    h->pend_have_next = false;
    for (int r = 0; r < h->dp_world; ++r) {
        const int32_t* ids_r = h->xg_ids + (size_t)r * rows * F;
        fnn_handle::SortSlot& sl = h->slot[h->cur];
        {
            ProfScope ps(h, "sort_now", h->st);
            SortArgs so{ids_r, rows, F, h->n_rows, sl.rec, sl.owner_cnt, F, h->skeys, h->tag_first, sl.tag_shared, next_stamp(h, sl)};
            launch_sort16(h, so);
        }
        launch_steps23<T>(h, make_roles(h, false, true, false, h->xg_gxp + (size_t)r * rows * h->K1p));
    }
    HIPCHK(h, hipGetLastError());
    return FNN_OK;
}

// gx in the reference's layout, for a caller that asked for it
void copy_gx_out(fnn_handle* h, int B, float* gx_out_dev)
{
    const size_t n = (size_t)B * h->xdim;
    if (h->bag) hipLaunchKernelGGL(k_copy_cols, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->gx_raw, h->K1p, B, h->xdim, gx_out_dev);
    else hipLaunchKernelGGL(k_gx_ref, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->gxp, h->K1p, B, h->F, h->K, h->rw,
                            h->wide ? h->F * h->rw : h->K, gx_out_dev);
}

// The fast path: three role-split launches on the main stream (fnn_step_kernels.hip.h).
template <typename T>
int run_step_fast(fnn_handle* h, const int32_t* ids, const float* y, int B, const uint8_t* m1,
                  const uint8_t* m2, float* p_out, float* gx_out_dev, bool update)
{
    const bool native = update && h->dp;                                     // the step runs its own collective
    const bool local = !native || h->dp_sparse == FNN_DP_SPARSE_LOCAL;      // else EXCHANGE: the rows are grouped over the GLOBAL batch later
    // grouping of THIS batch: done by the previous step (fnn_prefetch_ids) or right now
    if (!local) { h->next_ids = nullptr; h->next_B = 0; }
    else if (!(h->sorted_ids == ids && h->sorted_B == B)) {
        h->prefetch_misses++;
        ProfScope ps(h, "sort_now", h->st);
        fnn_handle::SortSlot& sl = h->slot[h->cur];
        launch_sort16(h, SortArgs{ids, B, h->F, h->n_rows, sl.rec, sl.owner_cnt, h->F, h->skeys, h->tag_first, sl.tag_shared, next_stamp(h, sl)});
    } else h->prefetch_hits++;
    h->pend_Ba = rup(B, 256);
    h->pend_have_next = h->next_ids != nullptr && !(h->next_ids == ids && h->next_B == B);
    { ProfScope pe(h, "empty", h->st); }         // a back-to-back event pair: what the event mechanism itself adds to every slot
    {
        ProfScope ps(h, "step1", h->st);
        MlpArgs<T> ma = make_mlp_args<T>(h, ids, y, B, m1, m2, true, p_out);
        if (h->bag && gx_out_dev) ma.gx_raw = h->gx_raw;
        launch_step1<T>(h, h->pend_Ba / 16, ma);
    }
    if (gx_out_dev) copy_gx_out(h, B, gx_out_dev);
    if (!native) {
        // single: dense and sparse roles share the launches; split API (no update): the sparse half is deferred to fnn_step_scatter
        launch_steps23<T>(h, make_roles(h, true, update, update));
        if (!update) h->scatter_pending = true;
    } else if (!dp_bucket_mode(h)) {
        // slabs collective: the same launches with ONE collective between the second and the third -- the split-K slabs of the
        // weight gradients are all-reduced in place, the third launch then sums GLOBAL slabs
        const StepRoles r = make_roles(h, true, local, true);
        launch_step2<T>(h, r);
        RCCHK(dp_allreduce(h, h->slab, (size_t)h->splitk * h->nslab, "weight-gradient slabs"));
        launch_step3<T>(h, r);
    } else {
        // bucket collective: launch 3 sums this rank's slabs (no update), the collective carries a quarter of the bytes, a fourth
        // launch applies the update -- with the p2p collective that launch IS the all-reduce
        const bool p2p = h->dp_collective == FNN_DP_COLLECTIVE_P2P;
        launch_steps23<T>(h, make_roles(h, true, local, false, nullptr, p2p ? p2p_bucket(h) : nullptr));
        RCCHK(dp_finish_bucket<T>(h, p2p));
    }
    if (!local) {
        h->pend_have_next = false;
        RCCHK(dp_exchange_sparse<T>(h, ids, B));
    }
    HIPCHK(h, hipGetLastError());
    return FNN_OK;
}

// ---- the generic path, one kernel per layer / stage, any padded shape, B up to 16384: its stages, then run_step
// A3, A4 and the head: gather, d1 = act(x' W1p) * r1, d2 = tanh(d1 W2p) * r2 (predict: acti_type, no mask), output unit, loss, delta2
template <typename T>
void layers_forward(fnn_handle* h, const int32_t* ids, const float* y, int B, int Ba, const uint8_t* m1, const uint8_t* m2, bool train, float* p_out)
{
    const int K1p = h->K1p, H1p = h->H1p, H2p = h->H2p, ldT = h->ldT;
    T *xp = (T*)h->xp, *d1 = (T*)h->d1, *d2 = (T*)h->d2;
    {
        ProfScope ps(h, "gather", h->st);
        if (h->wide) {
            const int nthreads = Ba / 4 * (K1p / 4);
            hipLaunchKernelGGL((k_gather_wide<T>), dim3((nthreads + 255) / 256), dim3(256), 0, h->st, ids, B, Ba,
                               h->F, h->rw, h->table16, h->n_rows, h->w0, xp, K1p, (T*)h->xpT, ldT, h->err_flag);
        } else {
            const int nthreads = Ba * h->F;
            hipLaunchKernelGGL((k_gather<T>), dim3((nthreads + 255) / 256), dim3(256), 0, h->st, ids, B, Ba,
                               h->F, h->K, h->table16, h->n_rows, h->w0, xp, K1p, (T*)h->xpT, ldT, h->err_flag);
        }
    }
    {
        ProfScope ps(h, "fwd1", h->st);
        EpiFwd<T> e{d1, H1p, train ? (T*)h->d1T : nullptr, ldT, m1, h->cfg.act, h->H1, B};
        launch_gemm<T, 4>(h->st, xp, K1p, (const T*)h->w1t, Ba, H1p, K1p, e);
    }
    {
        ProfScope ps(h, "fwd2", h->st);
        EpiFwd<T> e{d2, H2p, train ? (T*)h->d2T : nullptr, ldT, m2, train ? ACT_TANH : h->cfg.act, h->H2, B};
        launch_gemm<T, 4>(h->st, d1, H1p, (const T*)h->w2t, Ba, H2p, H1p, e);
    }
    ProfScope ps(h, "head", h->st);
    hipLaunchKernelGGL((k_head<T>), dim3(Ba / 64), dim3(256), 0, h->st, d2, H2p, h->H2, h->master + h->nw12, m2, y, B, train ? 1 : 0,
                       p_out, (T*)h->dl2, (T*)h->dl2T, ldT, (T*)h->dl3T, h->loss_t);
}
// A5, backward data: delta1 = (delta2 W2p^T) * r1 * act'(d1), then gx' = delta1 W1p^T
template <typename T> void layers_backward(fnn_handle* h, int B, int Ba, const uint8_t* m1)
{
    const int K1p = h->K1p, H1p = h->H1p, H2p = h->H2p;
    {
        ProfScope ps(h, "bwd1", h->st);
        EpiBwd<T> e{(T*)h->dl1, H1p, (T*)h->dl1T, h->ldT, (T*)h->d1, m1, h->cfg.act, h->H1, B};
        launch_gemm<T, 4>(h->st, (T*)h->dl2, H2p, (const T*)h->w2, Ba, H1p, H2p, e);
    }
    ProfScope ps(h, "gx", h->st);
    EpiF32 e{h->gxp, K1p, 0};
    launch_gemm<T, 4>(h->st, (T*)h->dl1, H1p, (const T*)h->w1, Ba, K1p, H1p, e);
}
// A5, dense gradients: contraction over the examples into split-K slabs, then their sum (+ L2 term) into the bucket
template <typename T> int layers_wgrad_reduce(fnn_handle* h, int Ba)
{
    {
        ProfScope ps(h, "wgrad", h->st);
        const WgradArgs wa = make_wgrad_args<T>(h, Ba);
        const dim3 grid(wgrad_blocks(wa), h->splitk);
        bool lds_form = false;
        if constexpr (sizeof(T) == 2) {
            if (h->wgrad_lds) {
                hipLaunchKernelGGL((k_wgrad<T, WGRAD_LDS>), grid, dim3(256), WGRAD_LDS_BYTES, h->st, wa);
                lds_form = true;
            }
        }
        if (!lds_form) hipLaunchKernelGGL((k_wgrad<T>), grid, dim3(256), 0, h->st, wa);
    }
    // native data parallelism, slabs payload: the SAME collective as the three-launch path issues, so that a rank whose shard
    // takes these kernels (shadowed features, B > 4096) pairs with peers that do not
    if (h->step_native_dp && !dp_bucket_mode(h)) RCCHK(dp_allreduce(h, h->slab, (size_t)h->splitk * h->nslab, "weight-gradient slabs"));
    ProfScope ps(h, "reduce", h->st);
    hipLaunchKernelGGL(k_reduce, dim3((unsigned)((h->nw + 255) / 256 + 1)), dim3(256), 0, h->st, h->slab, h->splitk, h->nw, h->nw12,
                       h->nslab, h->master, h->cfg.lambda1, h->cfg.reg_all, h->loss_t, Ba, h->bucket, h->loss_dev);
    return FNN_OK;
}
// A6 part 2: the two-level row update on the grouping in `sl`
void layers_row_update(fnn_handle* h, const fnn_handle::SortSlot& sl, int N2)
{
    ScatArgs sa = make_scat_args(h, sl, N2);
    if (h->wide) sa.gxf = h->rw;                             // rows of rw floats: chunks of WCH entries, a 16-byte piece per thread
    {
        ProfScope ps(h, "scatter", h->st);
        // narrow rows: a thread per live quarter-column of a chunk of 16 entries (or 16 lanes per chunk); scat1_blocks settles sa.form
        const int nblk = h->wide ? (int)(((size_t)h->F * (N2 / WCH) * (h->rw / 4) + 255) / 256) : scat1_blocks(sa, h->kn.scat_form);
        if (h->wide) hipLaunchKernelGGL(k_scatdw1, dim3(nblk), dim3(256), 0, h->st, sa);
        else hipLaunchKernelGGL(k_scat1, dim3(nblk), dim3(256), 0, h->st, sa);
    }
    ProfScope ps(h, "finalize", h->st);
    if (h->wide) hipLaunchKernelGGL(k_scatdw2, dim3(256), dim3(256), 0, h->st, sa);
    else hipLaunchKernelGGL(k_scat2, dim3(64), dim3(256), 0, h->st, sa);
}

template <typename T>
int run_step(fnn_handle* h, const int32_t* ids, const float* y, int B, const uint8_t* m1,
             const uint8_t* m2, bool train, float* p_out, float* gx_out_dev)
{
    const int Ba = rup(B, 256);
    // shadowed features join their field's keys behind the B regular ones: room for all of them in any one field
    const int nsh = train ? h->n_shadow : 0;
    const int N2 = sort_n2(B + nsh);
    if (nsh > 0) {
        if (B + nsh > 16384) FAIL(h, FNN_ERR_ARG, "batch plus shadowed features exceed 16384 keys per field");
        RCCHK(ensure_global_ws(h, B + nsh));                   // the per-batch slots hold max_batch keys per field
    }
    fnn_handle::SortSlot& sl = nsh > 0 ? h->gsl : h->slot[h->cur];
    h->sorted_ids = nullptr; h->next_ids = nullptr;            // this path keeps no grouping across steps
    if (h->bag && !h->strip_ok) FAIL(h, FNN_ERR_ARG, "FNN_MODE_BAG runs on the strip kernel only, which FNN_NO_FUSE=1 turns off (hidden1 256..319 with hidden2 64..127, or <= 63 / <= 63 at h0 <= 252)");
    if (h->bag && train) FAIL(h, FNN_ERR_ARG, "FNN_MODE_BAG trains through the three-launch path only (B <= 4096)");
    if (train && h->step_native_dp && h->dp_sparse == FNN_DP_SPARSE_EXCHANGE)
        FAIL(h, FNN_ERR_ARG, "FNN_DP_SPARSE_EXCHANGE runs on the three-launch path only (B <= 4096, hidden sizes the strip kernel is built for)");
    if (train) {   // A6 part 1: group the (row, t) pairs
        ProfScope ps(h, "sort", h->st);
        launch_k_sort(h->st, N2, ids, B, h->F, h->n_rows, sl, h->shadow_dev, h->n_shadow, h->err_flag);
    }
    if (h->strip_ok) {
        ProfScope ps(h, "mlp", h->st);
        launch_step1<T>(h, Ba / 16, make_mlp_args<T>(h, ids, y, B, m1, m2, train, p_out));
    } else layers_forward<T>(h, ids, y, B, Ba, m1, m2, train, p_out);
    if (!train) return FNN_OK;
    if (!h->strip_ok) layers_backward<T>(h, B, Ba, m1);
    RCCHK(layers_wgrad_reduce<T>(h, Ba));
    if (gx_out_dev) copy_gx_out(h, B, gx_out_dev);
    layers_row_update(h, sl, N2);
    HIPCHK(h, hipGetLastError());
    return FNN_OK;
}

// Workspaces for the grouping and the two-level update of a GLOBAL batch of up to N2 (row, t) pairs per field: the per-rank
// slots are sized for max_batch, a global batch is world times that.  Grown on demand (the first call synchronises).
int ensure_global_ws(fnn_handle* h, int B_g)
{
    int N2 = sort_n2(B_g);
    if (N2 <= h->gN2 && h->cpow_cap >= B_g + 1) return FNN_OK;
    HIPCHK(h, hipStreamSynchronize(h->st));
    if (N2 > h->gN2) {
        fnn_handle::SortSlot& sl = h->gsl;
        row_group_free(sl);
        HIPCHK(h, row_group_alloc(sl, h->F, N2, h->wide, h->wide ? h->rw : SLOT, h->st));
        h->gN2 = N2;
    }
    if (h->cpow_cap < N2 + 1) {             // a row can be hit by every example of the global batch
        hipFree(h->cpow_dev); h->cpow_dev = nullptr;
        h->cpow_cap = N2 + 1;
        RCCHK(alloc_dev(h, &h->cpow_dev, (size_t)h->cpow_cap));
        h->cpow_c = -1.0; h->cpow_n = 0;
        if (h->step_bsize > 0) RCCHK(update_cpow(h, h->step_bsize, B_g));
    }
    HIPCHK(h, hipStreamSynchronize(h->st));
    return FNN_OK;                              // (the LDS attributes of k_sort<8> / <16> are set at fnn_create)
}

// sparse-row SGD of a global batch in global example order (python/FNN_wnzh.py:299-306): one grouping per field over the
// global (row, t) keys -- the one-workgroup bitonic sort up to 16,384 keys, the library's own radix sort (metrics.hip) beyond -- then the
// two-level segmented update reading the gathered gradients
int scatter_global_impl(fnn_handle* h, const int32_t* ids_g, const float* gxp_g, int B_g)
{
    RCCHK(ensure_global_ws(h, B_g));
    if (h->cpow_n < B_g + 1) FAIL(h, FNN_ERR_STATE, "decay table shorter than the global batch");
    fnn_handle::SortSlot& sl = h->gsl;
    const int N2 = sort_n2(B_g), F = h->F;
    {
        ProfScope ps(h, "sort_global", h->st);
        if (N2 > 16384) {
            std::string err;
            if (group_global(h->st, ids_g, B_g, F, h->n_rows, N2, sl.rec, sl.owner_cnt, &h->gws, &h->gws_bytes, err) != 0)
                FAIL(h, FNN_ERR_HIP, err);
        } else launch_k_sort(h->st, N2, ids_g, B_g, F, h->n_rows, sl, nullptr, 0, h->err_flag);
    }
    {
        ProfScope ps(h, "scatter_global", h->st);
        ScatArgs sa = make_scat_args(h, sl, N2);
        sa.gxp = gxp_g;
        launch_scat_narrow(h->st, sa, h->kn.scat_form, N2 > 4096 ? 256 : 64);      // after sa.gxp changed: the caller's buffer may not be 16-byte aligned
    }
    HIPCHK(h, hipGetLastError());
    h->next_ids = nullptr; h->next_B = 0;       // no grouping of a later batch rides on this step
    h->scatter_pending = false;
    return FNN_OK;
}

// ---- RCCL, opened at run time: librccl.so.1 is already in the process under PyTorch-ROCm (RTLD_NOLOAD finds that copy: one
// RCCL per process), otherwise the loader's search path / this library's RUNPATH (/opt/rocm) finds it.
struct RcclApi {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
RcclApi g_rccl;

int rccl_load(std::string& err)
{
    static std::mutex mu;                          // handles of several host threads may set up data parallelism at once
    std::lock_guard<std::mutex> lock(mu);
    if (g_rccl.lib) return FNN_OK;
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) { err = std::string("cannot open librccl.so.1: ") + dlerror(); return FNN_ERR_HIP; }
    RcclApi a; a.lib = lib;
#define RSYM(f) do { a.f = reinterpret_cast<decltype(a.f)>(dlsym(lib, "nccl" #f)); if (!a.f) { err = "librccl: symbol nccl" #f " not found"; return FNN_ERR_HIP; } } while (0)
    RSYM(GetUniqueId); RSYM(CommInitRank); RSYM(AllReduce); RSYM(AllGather); RSYM(CommDestroy); RSYM(GetErrorString);
#undef RSYM
    g_rccl = a;
    return FNN_OK;
}

int rccl_allreduce_cb(void* ctx, float* buf, int64_t n, void* stream)
{
    fnn_handle* h = static_cast<fnn_handle*>(ctx);
    const ncclResult_t r = g_rccl.AllReduce(buf, buf, (size_t)n, ncclFloat32, ncclSum, h->comm, (hipStream_t)stream);
    if (r != ncclSuccess) { h->err = std::string("ncclAllReduce: ") + g_rccl.GetErrorString(r); return -1; }
    return 0;
}
int rccl_allgather_cb(void* ctx, const void* send, void* recv, int64_t bytes, void* stream)
{
    fnn_handle* h = static_cast<fnn_handle*>(ctx);
    const ncclResult_t r = g_rccl.AllGather(send, recv, (size_t)bytes, ncclInt8, h->comm, (hipStream_t)stream);
    if (r != ncclSuccess) { h->err = std::string("ncclAllGather: ") + g_rccl.GetErrorString(r); return -1; }
    return 0;
}

void p2p_release(fnn_handle* h)
{
    for (int r = 0; r < 8; ++r) {
        if (h->peer_opened[r] && h->peer[r]) hipIpcCloseMemHandle(h->peer[r]);
        h->peer[r] = nullptr; h->peer_opened[r] = false;
    }
    if (h->xr) hipFree(h->xr);
    if (h->p2p_wait_max) { hipFree(h->p2p_wait_max); h->p2p_wait_max = nullptr; }
    h->xr = nullptr; h->xr_kind = 0; h->p2p_attached = false; h->dp_step_no = 0;
    if (h->dp_collective == FNN_DP_COLLECTIVE_P2P) h->dp_collective = FNN_DP_COLLECTIVE_CALLBACK;
}

int dp_setup(fnn_handle* h, int rank, int world, int sparse_mode)
{
    if (world < 1 || rank < 0 || rank >= world) FAIL(h, FNN_ERR_ARG, "fnn_dp_init: rank / world out of range");
    if (sparse_mode != FNN_DP_SPARSE_LOCAL && sparse_mode != FNN_DP_SPARSE_EXCHANGE) FAIL(h, FNN_ERR_ARG, "fnn_dp_init: bad sparse_mode");
    if (h->in_step) FAIL(h, FNN_ERR_STATE, "fnn_dp_init inside a step");
    if (sparse_mode == FNN_DP_SPARSE_EXCHANGE) {
        if (h->wide) FAIL(h, FNN_ERR_ARG, "FNN_DP_SPARSE_EXCHANGE: not supported on wide rows (k >= 17; its exchange carries 16-float slots): use FNN_DP_SPARSE_LOCAL");
        if ((int64_t)world * h->ldT > GLOBAL_BATCH_MAX) FAIL(h, FNN_ERR_ARG, "FNN_DP_SPARSE_EXCHANGE: world * max_batch (rounded up to 256) must be <= 32768");
        if (h->Bmax > h->three_launch_max_B) FAIL(h, FNN_ERR_ARG, "FNN_DP_SPARSE_EXCHANGE runs on the three-launch path only (max_batch <= 4096, hidden sizes the strip kernel is built for)");
        const size_t rows = (size_t)h->ldT;
        if (!h->xg_ids_send) RCCHK(alloc_dev(h, &h->xg_ids_send, rows * h->F));
        if (h->xg_ids) { hipFree(h->xg_ids); h->xg_ids = nullptr; }
        if (h->xg_gxp) { hipFree(h->xg_gxp); h->xg_gxp = nullptr; }
        RCCHK(alloc_dev(h, &h->xg_ids, rows * world * h->F));
        RCCHK(alloc_dev(h, &h->xg_gxp, rows * world * h->K1p));
        if (!h->bag) RCCHK(ensure_global_ws(h, (int)rows * world));
    }
    h->dp_rank = rank; h->dp_world = world; h->dp_sparse = sparse_mode;
    h->sorted_ids = nullptr; h->next_ids = nullptr;
    h->dp_payload = FNN_DP_PAYLOAD_SLABS; h->dp_collective = FNN_DP_COLLECTIVE_CALLBACK;
    if (const char* ev = getenv("FNN_DP_PAYLOAD")) {
        if (!strcmp(ev, "bucket")) h->dp_payload = FNN_DP_PAYLOAD_BUCKET;
        else if (strcmp(ev, "slabs") != 0) FAIL(h, FNN_ERR_ARG, "FNN_DP_PAYLOAD must be slabs or bucket");
    }
    return FNN_OK;
}

int check_ready(fnn_handle* h, int B) {
    if (!h) return FNN_ERR_ARG;
    if (B <= 0 || B > h->Bmax) FAIL(h, FNN_ERR_ARG, "B must be in [1, max_batch]");
    if (!h->table16) FAIL(h, FNN_ERR_STATE, "fnn_set_table has not been called");
    if (!(h->dense_set[0] && h->dense_set[1] && h->dense_set[2]))
        FAIL(h, FNN_ERR_STATE, "fnn_set_dense has not been called for all three layers");
    return FNN_OK;
}

// every knob fnn_create takes from the environment, each with the values it accepts; anything else leaves the default
FnnKnobs read_knobs(bool bag)
{
    FnnKnobs k;
    if (const char* e = getenv("FNN_WT_STORES")) k.wt_stores = atoi(e);
    if (const char* e = getenv("FNN_STEP1_WAVES")) k.step1_waves = atoi(e) == 4 ? 4 : 8;
    if (const char* e = getenv("FNN_STEP1_FORM")) k.step1_fixed = strcmp(e, "generic") != 0;      // fixed | generic; anything else: the default, fixed
    if (const char* e = getenv("FNN_NO_FUSE")) k.fused = !(e[0] == '1');
    if (const char* e = getenv("FNN_ROLE_OFF")) k.role_off = atoi(e);
    if (const char* e = getenv("FNN_SPLITK")) { const int v = atoi(e); if (v == 2 || v == 4 || v == 8 || v == 16) k.splitk = v; }   // tuning knob
    if (const char* e = getenv("FNN_SCAT2_WGS")) { const int v = atoi(e); if (v >= 16 && v <= 1024) k.scat2_wgs = v; }
    k.wgrad_form = wgrad_form_env(); k.scat_form = scat1_form_env(); k.scat2_form = scat2_form_env();
    k.sort_merge4 = sort_merge4_env(bag ? 0 : 1);
    return k;
}

// the shapes and the paths of a handle, from a configuration fnn_create has checked (plan_step1 / plan_keys add the kernels)
FnnPlan make_plan(const fnn_cfg& c, const FnnKnobs& kn)
{
    FnnPlan p;
    p.F = c.n_fields; p.K = c.k; p.H1 = c.hidden1; p.H2 = c.hidden2;
    p.xdim = 1 + p.F * p.K;
    p.K1p = rup(p.F * SLOT, 64); p.H1p = rup(p.H1 + 1, 64); p.H2p = rup(p.H2 + 1, 64);
    p.bag = c.mode == FNN_MODE_BAG;
    if (p.bag) { p.rw = c.h0; p.K = c.h0; p.xdim = c.h0; p.K1p = rup(c.h0 + 1, 64); }
    p.wide = !p.bag && p.K >= 17;
    if (p.wide) { p.rw = rup(p.K, 4); p.K1p = rup(p.F * p.rw + 2, 64); }       // field columns, then w_0 and the ones column
    p.Bmax = c.max_batch; p.ldT = rup(p.Bmax, 256);
    p.N2max = SORT_N; while (p.N2max < p.Bmax) p.N2max <<= 1;    // the three-launch path groups SORT_N slots per field whatever max_batch is
    p.n1 = (size_t)p.K1p * p.H1p; p.n2 = (size_t)p.H1p * p.H2p;
    p.nw12 = p.n1 + p.n2; p.nw = p.nw12 + p.H2p;
    p.off_bag = p.nw12 + (size_t)p.H2p * 64;
    p.nbag = p.bag ? (size_t)p.K1p : 0;
    p.nslab = p.off_bag + p.nbag * 64;
    p.bf16 = c.precision == FNN_PREC_BF16; p.split = c.precision == FNN_PREC_BF16X3;
    p.strip_shape = strip_shape_ok(p);
    p.strip_ok = kn.fused && p.strip_shape;
    p.three_launch_max_B = p.strip_ok ? SORT_N : 0;
    // Split-K and the form of the weight-gradient products (the measurements: DESIGN.md section 4, "The step's host side").
    // eight: handles whose every step takes the three launches with the quarter-column or half-chunk scatter role beside the
    // products in launch 2 (FM rows, f32 and bf16, max_batch <= 4096); everything else four -- the layer-by-layer kernels, bag mode,
    // the bf16 pairs, the slot-per-lane role.  lds_dflt: the same handles in bf16, where a slice of the handle's largest batch at
    // split-K 4 holds a whole stage (max_batch > 256), stage the products' operands through LDS, which buys split-K 4 again.  An
    // explicit FNN_WGRAD_FORM=lds takes the form anywhere in bf16 and moves no split-K; FNN_SPLITK overrules the split.
    const bool eight = p.strip_ok && !p.bag && kn.scat_form != SCAT1_SLOT && !p.split && p.Bmax <= SORT_N;
    const bool lds_dflt = kn.wgrad_form == -1 && eight && p.bf16 && p.ldT / 4 / Traits<bf16_t>::KS >= WGRAD_LDS_S;
    p.wgrad_lds = kn.wgrad_form == WGRAD_LDS || lds_dflt ? 1 : 0;
    p.splitk = kn.splitk ? kn.splitk : (eight && !lds_dflt ? 8 : 4);
    // a slice of the shortest padded batch (256 lines) must hold a k-step of the element type, or the products of a batch of up to
    // 256 lines walk no step and the dense tensors do not move: FNN_SPLITK=16 means 8 in bf16 (32 lines a step)
    if (p.bf16) p.splitk = std::min(p.splitk, 256 / Traits<bf16_t>::KS);
    return p;
}

// ---- fnn_train_step_multi / fnn_bag_train_step_multi: one step of several handles on one feed (the kernels: k_gstep1 / k_gstep2 / k_gstep3)
// A call on a list of handles: GroupCall (group_call.h), refusals without a usable hs[0] left with fnn_last_error(NULL).
using FnnGroup = GroupCall<fnn_handle>;

// What decides which handles one set of group launches serves: the three kernels with their block and LDS sizes, and what
// shapes the grid -- a LAUNCH CLASS (include/fnn_hip.h).  The kernels follow from element type, padded shapes, key width, sort
// runs, weight-gradient form and the strip kernel's knobs (gstep*_sel).  Bag mode: `bag` itself; K is the width of a bag row (rw =
// h0, which with K1p tells h0 192..252 from 256..316 and sizes level 1 of the row update) and F the columns of a line (2..64).
// Key width and sort runs choose the kernels of launches 2 and 3, so members that agree in k[] agree in them.
struct LaunchClass {
    FnnKernel<> k[3]; int prec, bag, F, K, K1p, H1p, H2p, splitk, wl, scat_form, scat2_form, scat2_wgs, wt_stores, role_off;
    std::vector<int> members;                      // indices into hs, in the call's order
    bool same(const LaunchClass& o) const
    {
        for (int i = 0; i < 3; ++i) if (k[i].fn != o.k[i].fn || k[i].threads != o.k[i].threads || k[i].lds != o.k[i].lds) return false;
        return prec == o.prec && bag == o.bag && F == o.F && K == o.K && K1p == o.K1p && H1p == o.H1p && H2p == o.H2p && splitk == o.splitk && wl == o.wl &&
               scat_form == o.scat_form && scat2_form == o.scat2_form && scat2_wgs == o.scat2_wgs && wt_stores == o.wt_stores && role_off == o.role_off;
    }
};
template <typename T> LaunchClass launch_class_of(const fnn_handle* h)
{
    const bool m4 = h->kn.sort_merge4 != 0;
    const bool wl = !(h->kn.role_off & 2) && h->wgrad_lds && sizeof(T) == 2;       // launch_step2's choice
    const GroupKernel<T> k1 = h->bag ? gstep1_bag_sel<T>(*h, h->kn) : gstep1_sel<T>(*h, h->kn), k2 = gstep2_sel<T>(h->key64, m4, wl), k3 = gstep3_sel<T>(h->key64, m4);
    LaunchClass c{};
    c.k[0] = {reinterpret_cast<void (*)()>(k1.fn), k1.threads, k1.lds};
    c.k[1] = {reinterpret_cast<void (*)()>(k2.fn), k2.threads, std::max(k2.lds, wl ? WGRAD_LDS_BYTES : (size_t)0)};
    c.k[2] = {reinterpret_cast<void (*)()>(k3.fn), k3.threads, k3.lds};
    c.prec = h->cfg.precision; c.bag = h->bag ? 1 : 0; c.F = h->F; c.K = h->K; c.K1p = h->K1p; c.H1p = h->H1p; c.H2p = h->H2p; c.splitk = h->splitk; c.wl = wl;
    c.scat_form = h->kn.scat_form; c.scat2_form = h->kn.scat2_form; c.scat2_wgs = h->kn.scat2_wgs; c.wt_stores = h->kn.wt_stores;
    c.role_off = h->kn.role_off;
    return c;
}
// Member h's entry of the argument array: what launch_step1 / launch_step2 / launch_step3 would pass for it, with the grouping
// class's grouping (`grp`: the slot in which the class's first member holds the batch's): its records and, in bag mode, its marks
// of the rows that several columns of the batch hold, with the stamp they were written under -- a follower's own tag_shared / stamp
// are those of some earlier batch, and with them a shared row would take the plain store and keep one column's sum of all.
// x2 / x3: the workgroups it needs in launches 2 / 3.
template <typename T>
bool fill_group_arg(fnn_handle* h, const fnn_handle::SortSlot& grp, const int32_t* ids, const float* y, int B, const uint8_t* m1, const uint8_t* m2,
                    float* p_out, GroupPack* pack, void* dst, int* x2, int* x3)
{
    GroupArg<T>& g = *static_cast<GroupArg<T>*>(dst);
    const StepRoles r = make_roles(h, true, true, true);
    g.ma = make_mlp_args<T>(h, ids, y, B, m1, m2, true, p_out);
    g.nmlp = h->pend_Ba / 16;
    Step23Args a = make_step23_args(h, r, false);
    a.sa.rec = grp.rec; a.sa.tag_shared = grp.tag_shared; a.sa.stamp = grp.stamp;
    g.wa = make_wgrad_args<T>(h, h->pend_Ba);
    g.nwx = r.dense ? wgrad_blocks(g.wa) : 0; g.splitk = h->splitk;
    g.nsc1 = !r.sparse ? 0 : (h->bag ? (int)(((size_t)h->F * (SORT_N / WCH) * (h->rw / 4) + 255) / 256)      // launch_step2's count
                                     : scat1_blocks(a.sa, h->kn.scat_form));
    g.so2 = a.so; g.sa = a.sa;
    g.so3 = make_step23_args(h, r, true).so;
    g.ta = make_tail_args(h, r);
    g.nsc2 = r.sparse ? h->kn.scat2_wgs : 0;
    g.pack = pack;
    *x2 = g.so2.nblk + g.nwx * g.splitk + g.nsc1;
    *x3 = g.so3.nblk + g.ta.nblk_red + g.nsc2;
    return a.have_next;
}
template <typename T> void launch_group(const LaunchClass& c, hipStream_t st, const void* dev_args, int nmlp, int x2, int x3)
{
    const GroupArg<T>* d = static_cast<const GroupArg<T>*>(dev_args);
    const unsigned M = (unsigned)c.members.size();
    using Fn = void (*)(const GroupArg<T>*);
    hipLaunchKernelGGL(reinterpret_cast<Fn>(c.k[0].fn), dim3(nmlp, M), dim3(c.k[0].threads), c.k[0].lds, st, d);
    // (x a multiple of 8: every model's blocks start on the XCD a solo launch's start on, which keeps the weight-gradient deal XCD-aware)
    if (x2 > 0) hipLaunchKernelGGL(reinterpret_cast<Fn>(c.k[1].fn), dim3(rup(x2, 8), M), dim3(c.k[1].threads), c.k[1].lds, st, d);
    if (x3 > 0) hipLaunchKernelGGL(reinterpret_cast<Fn>(c.k[2].fn), dim3(x3, M), dim3(c.k[2].threads), c.k[2].lds, st, d);
}

// ---- fnn_predict_multi / fnn_eval_multi: the predictions (and metrics) of several handles on one feed (the kernel: k_gpredict)
// What the two calls read from the environment, per call: none of it changes a bit of any result.
struct EvalKnobs {
    int fb_len = 4096;          // FNN_EVAL_FEED_BATCH=256..65536, a multiple of 256: lines per feed batch (k_gpredict)
    bool model_fast = false;    // FNN_EVAL_ORDER=model: the model is the fast index of the grid (default: tile, the strips of one model adjacent)
    bool per_batch = false;     // FNN_EVAL_LAUNCH=batch: one launch per feed batch (default: span, one launch over all feed batches)
};
constexpr int EVAL_FEED_BATCH_MAX = 65536;
EvalKnobs read_eval_knobs()
{
    EvalKnobs k;
    if (const char* e = getenv("FNN_EVAL_FEED_BATCH")) { const int v = atoi(e); if (v >= 256 && v <= EVAL_FEED_BATCH_MAX && v % 256 == 0) k.fb_len = v; }
    if (const char* e = getenv("FNN_EVAL_ORDER")) k.model_fast = !strcmp(e, "model");
    if (const char* e = getenv("FNN_EVAL_LAUNCH")) k.per_batch = !strcmp(e, "batch");
    return k;
}
// A member whose prediction is the strip kernel on FM rows rides in a group launch; every other one (bag mode, wide rows, shapes
// off the strip kernel, FNN_NO_FUSE) runs its own prediction launches inside the call.
inline bool pred_in_group(const fnn_handle* h) { return h->strip_ok && !h->bag; }
// The members that one k_gpredict launch serves: a launch class of the prediction -- element type, padded shapes and waves per
// strip, which is what gpredict_sel (as step1_sel(train = false)) looks at.  members: positions in the group, in its order.
struct PredClass { FnnKernel<> k; int prec; std::vector<int> members; };
template <typename T> PredClass pred_class_of(const fnn_handle* h)
{
    const GroupPredKernel<T> k = gpredict_sel<T>(*h, h->kn);
    return PredClass{{reinterpret_cast<void (*)()>(k.fn), k.threads, k.lds}, h->cfg.precision, {}};
}
// (y: the zeroed labels of one feed batch.  The strip kernel reads a.y[t] for every t < a.B while it predicts too and uses none
// of the values when train = 0 -- the solo path points it at the handle's loss_t for the same reason, which is only max_batch long)
template <typename T> void fill_pred_arg(fnn_handle* h, int m, const int32_t* ids, const float* y, int fb_len, float* p, void* dst)
{
    GroupPredArg<T>& g = *static_cast<GroupPredArg<T>*>(dst);
    g.ma = make_mlp_args<T>(h, ids, y, fb_len, nullptr, nullptr, false, p);
    g.m = m;
}
// One class's launches: the whole feed in one (up to 2^22 strips, 2^26 lines, a launch: the runtime counts a grid's threads in 32 bits), or one per feed batch.
template <typename T> void launch_gpredict(const PredClass& c, hipStream_t st, const void* dev_args, int64_t N, const EvalKnobs& ek)
{
    using Fn = void (*)(const GroupPredArg<T>*, int, int64_t, int, int64_t, int64_t, int);
    const GroupPredArg<T>* d = static_cast<const GroupPredArg<T>*>(dev_args);
    const int M = (int)c.members.size();
    const int64_t strips = (N + 15) / 16, span = ek.per_batch ? ek.fb_len / 16 : (int64_t)1 << 22;
    for (int64_t s0 = 0; s0 < strips; s0 += span) {
        const int64_t ns = std::min(span, strips - s0);
        dim3 grid((unsigned)ns, (unsigned)M);
        if (ek.model_fast) {
            const int64_t total = ns * M, gx = std::min<int64_t>(total, (int64_t)1 << 22);
            grid = dim3((unsigned)gx, (unsigned)((total + gx - 1) / gx));
        }
        hipLaunchKernelGGL(reinterpret_cast<Fn>(c.k.fn), grid, dim3(c.k.threads), c.k.lds, st, d, M, N, ek.fb_len, s0, ns, ek.model_fast ? 1 : 0);
    }
}
// The range flags of the n members behind `args`, bit 1 of each handle's error word, into flags[their position]; then the bit is
// cleared (after every read: a handle may be listed twice).  One workgroup.
static __global__ __launch_bounds__(256) void k_gpred_flags(const GroupPredArg<float>* __restrict__ args, const int n, int* __restrict__ flags)
{
    for (int i = threadIdx.x; i < n; i += 256) flags[args[i].m] = *args[i].ma.err & 1;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) if (flags[args[i].m]) atomicAnd(args[i].ma.err, ~1);
}
// What both calls refuse, all of it before anything is launched or written.
int pred_check(const FnnGroup& g, const int32_t* ids, bool need_y, const int32_t* y, int64_t N, bool need_p, float* const* p_out)
{
    RCCHK(g.check_list(nullptr));                                 // a handle may be listed twice: reading is not a race
    fnn_handle* const* hs = g.hs;
    const int M = g.n;
    if (!ids || (need_y && !y)) return g.refuse(FNN_ERR_ARG, need_y ? "null ids or y" : "null ids");
    if (need_p && !p_out) return g.refuse(FNN_ERR_ARG, "null p_out");
    if (need_p) for (int m = 0; m < M; ++m) if (!p_out[m]) return g.refuse(FNN_ERR_ARG, g.at("null p_out", m));
    if (N < 1 || N > ((int64_t)1 << 30)) return g.refuse(FNN_ERR_ARG, "N must be in [1, 2^30]");
    for (int m = 0; m < M; ++m)
        if (hs[m]->bag && !hs[m]->strip_ok) return g.refuse(FNN_ERR_ARG, g.at("FNN_MODE_BAG runs on the strip kernel only, which FNN_NO_FUSE=1 turns off (or a shape it is not built for)", m));
    for (int m = 0; m < M; ++m) {
        const fnn_handle* h = hs[m];
        if (!h->table16) return g.refuse(FNN_ERR_STATE, g.at("fnn_set_table has not been called", m));
        if (!(h->dense_set[0] && h->dense_set[1] && h->dense_set[2])) return g.refuse(FNN_ERR_STATE, g.at("fnn_set_dense has not been called for all three layers", m));
        if (h->in_step) return g.refuse(FNN_ERR_STATE, g.at("inside fnn_step_begin / fnn_step_end", m));
    }
    return FNN_OK;
}
// The predictions of the n members hs[0 .. n) of group `g` on the N lines, p[m] each: the argument array into hs[0]'s ring, one
// set of launches per prediction launch class, then the members off the strip kernel one after the other, each in chunks of its
// own max_batch with its stream swapped for the group's.  *dev_args: the members' arguments on the device (k_gpred_flags).
int pred_forward(const FnnGroup& g, fnn_handle* const* hs, int n, int base, const int32_t* ids, int64_t N, float* const* p, const EvalKnobs& ek,
                 const GroupPredArg<float>** dev_args)
{
    fnn_handle* h0 = g.h0;
    const hipStream_t st = h0->st;
    std::vector<PredClass> cls;
    std::vector<int> own;
    for (int m = 0; m < n; ++m) {
        if (!pred_in_group(hs[m])) { own.push_back(m); continue; }
        PredClass c = BY_PREC_RC(hs[m], pred_class_of, (hs[m]));
        const size_t i = class_index(cls, c, [](const PredClass& a, const PredClass& b) {
            return a.k.fn == b.k.fn && a.k.threads == b.k.threads && a.k.lds == b.k.lds && a.prec == b.prec; });
        cls[i].members.push_back(m);
    }
    size_t slot = 0;
    HIPCHK(h0, ring_take(h0->eval_ring, (size_t)n, &slot));
    const size_t elem = h0->eval_ring.elem;
    char* a = h0->eval_ring.host_bytes(slot);
    const char* d = h0->eval_ring.dev_bytes(slot);
    size_t pos = 0;
    auto fill = [&](int m) { BY_PREC(hs[m], fill_pred_arg, (hs[m], m, ids, h0->eval_y, ek.fb_len, p[m], a + pos * elem)); ++pos; };
    for (const PredClass& c : cls) for (int m : c.members) fill(m);
    for (int m : own) fill(m);                                        // not launched from: their range flags are read through them
    HIPCHK(h0, ring_send(h0->eval_ring, slot, (size_t)n, st));
    pos = 0;
    for (const PredClass& c : cls) {
        BY_PREC(hs[c.members[0]], launch_gpredict, (c, st, d + pos * elem, N, ek));
        pos += c.members.size();
    }
    HIPCHK(h0, hipGetLastError());
    for (int m : own) {
        fnn_handle* h = hs[m];
        const int rc = on_stream(h, st, [&]() -> int {
            for (int64_t lo = 0; lo < N; lo += h->Bmax) {
                const int B = (int)std::min<int64_t>(h->Bmax, N - lo);
                RCCHK(BY_PREC_RC(h, run_step, (h, ids + lo * h->F, nullptr, B, nullptr, nullptr, false, p[m] + lo, nullptr)));
            }
            HIPCHK(h, hipGetLastError());
            return FNN_OK;
        });
        if (rc != FNN_OK) return g.member_failed(rc, h, base + m);
    }
    *dev_args = reinterpret_cast<const GroupPredArg<float>*>(d);
    return FNN_OK;
}
// the zeroed labels of the longest feed batch, hs[0]'s from its first group call on
int ensure_eval_y(fnn_handle* h0)
{
    if (h0->eval_y) return FNN_OK;
    HIPCHK(h0, hipMalloc((void**)&h0->eval_y, EVAL_FEED_BATCH_MAX * sizeof(float)));
    HIPCHK(h0, hipMemsetAsync(h0->eval_y, 0, EVAL_FEED_BATCH_MAX * sizeof(float), h0->st));
    return FNN_OK;
}

}  // namespace

extern "C" {

const char* fnn_version(void) { return "fnn_hip 0.2 (gfx950)"; }

uint64_t fnn_cfg_size(void) { return (uint64_t)sizeof(fnn_cfg); }

const char* fnn_last_error(const fnn_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

const char* fnn_scat2_form(void)
{
    const int f = scat2_form_env(-1);
    return f == SCAT2_BLOCK ? "block" : f == SCAT2_WAVE ? "wave" : "default";
}

const char* fnn_scat1_form(void)
{
    const int f = scat1_form_env(-1);
    return f == SCAT1_SLOT ? "slot" : f == SCAT1_QUARTER ? "quarter" : f == SCAT1_HALF ? "half" : "default";
}

int fnn_create(const fnn_cfg* cfg, fnn_handle** out)
{
    if (!cfg || !out) { g_create_err = "null argument"; return FNN_ERR_ARG; }
    *out = nullptr;
    if (cfg->n_fields < 2 || cfg->n_fields > 64) { g_create_err = "n_fields must be in [2, 64]"; return FNN_ERR_ARG; }
    if (cfg->mode != FNN_MODE_FM && cfg->mode != FNN_MODE_BAG) { g_create_err = "bad mode"; return FNN_ERR_ARG; }
    if (cfg->mode == FNN_MODE_BAG && (cfg->h0 < 192 || cfg->h0 > 316 || cfg->h0 % 4 != 0)) {
        g_create_err = "FNN_MODE_BAG: h0 must be a multiple of 4 in [192, 316] (the strip kernel is built for bag rows of 256 or 320 padded floats; the reference uses 200 and 300, python/SNN_RBM.py:25,53)"; return FNN_ERR_ARG; }
    if (cfg->mode == FNN_MODE_FM && (cfg->k < 1 || cfg->k > 128 || cfg->k == 16)) {
        g_create_err = "k = rank+1 must be in [1, 15] (two pad slots of the 16-float row carry w_0 and the bias) or in [17, 128] (wide rows of rup(k, 4) floats); k = 16 is not supported"; return FNN_ERR_ARG; }
    if (cfg->mode == FNN_MODE_FM && cfg->k >= 17 && cfg->n_fields * rup(cfg->k, 4) > WIDE_XW_MAX) {
        g_create_err = "k >= 17: n_fields * rup(k, 4) must be <= 4096 (the layer-one width of the wide-row path)"; return FNN_ERR_ARG; }
    if (cfg->hidden1 < 1 || cfg->hidden1 > 4095 || cfg->hidden2 < 1 || cfg->hidden2 > 255) { g_create_err = "hidden1 must be in [1, 4095], hidden2 in [1, 255]"; return FNN_ERR_ARG; }
    if (cfg->max_batch < 1 || cfg->max_batch > 16384) { g_create_err = "max_batch must be in [1, 16384] (per-field LDS sort)"; return FNN_ERR_ARG; }
    if (cfg->precision != FNN_PREC_F32 && cfg->precision != FNN_PREC_BF16 && cfg->precision != FNN_PREC_BF16X3) { g_create_err = "bad precision"; return FNN_ERR_ARG; }
    if (cfg->act < 0 || cfg->act > 2) { g_create_err = "bad act"; return FNN_ERR_ARG; }
    const FnnKnobs kn = read_knobs(cfg->mode == FNN_MODE_BAG);
    if (kn.wgrad_form == -2) { g_create_err = "FNN_WGRAD_FORM must be direct or lds"; return FNN_ERR_ARG; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_err = std::string("no HIP device: ") + hipGetErrorString(e) + " (libfnn_hip.so has no CPU fallback)";
        return FNN_ERR_HIP;
    }
    if (cfg->device < 0 || cfg->device >= ndev) { g_create_err = "device ordinal out of range"; return FNN_ERR_ARG; }
    fnn_handle* h = new fnn_handle();
    static_cast<FnnPlan&>(*h) = make_plan(*cfg, kn);
    h->cfg = *cfg; h->dev = cfg->device; h->kn = kn;
    auto fail = [&] { g_create_err = h->err; fnn_destroy(h); };        // the cleanup of every early return below
#define OWN(p, n, ...) RCCHK(alloc_owned(h, p, n, ##__VA_ARGS__), fail())
    HIPCHK(h, hipSetDevice(h->dev), fail());
    if (cfg->stream) { h->st = (hipStream_t)cfg->stream; h->own_stream = false; }
    else { HIPCHK(h, hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking), fail()); h->own_stream = true; }
    const size_t ts = tsize(h), Ba = h->ldT;
    OWN(&h->master, h->nw);
    OWN(&h->bucket, h->nw + h->nbag);
    OWN(&h->slab, (size_t)h->splitk * h->nslab);
    OWN((char**)&h->w1, h->n1 * ts);   OWN((char**)&h->w1t, h->n1 * ts);
    OWN((char**)&h->w2, h->n2 * ts);   OWN((char**)&h->w2t, h->n2 * ts);
    OWN((char**)&h->xp, Ba * h->K1p * ts);  OWN((char**)&h->xpT, Ba * h->K1p * ts);
    OWN((char**)&h->d1, Ba * h->H1p * ts);  OWN((char**)&h->d1T, Ba * h->H1p * ts);
    OWN((char**)&h->dl1, Ba * h->H1p * ts); OWN((char**)&h->dl1T, Ba * h->H1p * ts);
    OWN((char**)&h->d2, Ba * h->H2p * ts);
    OWN((char**)&h->dl2, Ba * h->H2p * ts); OWN((char**)&h->dl2T, Ba * h->H2p * ts);
    OWN(&h->gxp, Ba * h->K1p);
    OWN((char**)&h->d2T, Ba * h->H2p * ts);
    OWN((char**)&h->dl3T, Ba * 64 * ts);
    OWN(&h->loss_t, Ba);
    OWN(&h->loss_dev, (size_t)1);
    for (auto& sl : h->slot) HIPCHK(h, row_group_alloc(sl, h->F, h->N2max, h->bag || h->wide, h->rw, h->st), fail());
    if (h->bag) {
        if (!h->strip_shape) FAIL(h, FNN_ERR_ARG, "FNN_MODE_BAG needs hidden sizes the strip kernel is built for: hidden1 256..319 with hidden2 64..127 (e.g. 300/100) at any h0, or hidden1 <= 63 with hidden2 <= 63 at h0 <= 252", fail());
        OWN(&h->bb0, (size_t)h->K1p);
        OWN((char**)&h->dlxT, Ba * h->K1p * ts);
        OWN((char**)&h->onesT, Ba * 64 * ts);
        OWN(&h->gx_raw, Ba * h->K1p);
        // onesT: fragment-tiled [64][ldT] matrix whose row 0 is all ones (column sums via MFMA)
        std::vector<unsigned char> ones(Ba * 64 * ts, 0);
        for (size_t t = 0; t < Ba; ++t) {
            if (h->bf16) { const unsigned short one = 0x3F80; memcpy(&ones[ft_off<bf16_t>(0, (int)t, (int)Ba) * 2], &one, 2); }
            else if (h->split) { const bs16_t one(1.0f); memcpy(&ones[ft_off<bs16_t>(0, (int)t, (int)Ba) * 4], &one, 4); }
            else { const float one = 1.0f; memcpy(&ones[ft_off<float>(0, (int)t, (int)Ba) * 4], &one, 4); }
        }
        // alloc_dev zeroes with hipMemsetAsync on the handle's (non-blocking) stream, which a null-stream hipMemcpy does not
        // wait for: without this sync the zeroing could land AFTER the copy (seen as a bag bias that never moved, one run in a few)
        HIPCHK(h, hipStreamSynchronize(h->st), fail());
        HIPCHK(h, hipMemcpy(h->onesT, ones.data(), ones.size(), hipMemcpyHostToDevice), fail());
    }
    BY_PREC(h, plan_step1, (h));
    BY_PREC(h, plan_keys, (h, true));                                 // 64-bit keys until the table is set
    OWN((char**)&h->skeys, (size_t)h->F * SORT_N * 8);
    h->cpow_cap = h->N2max + 1;
    RCCHK(alloc_dev(h, &h->cpow_dev, (size_t)h->cpow_cap), fail());   // (regrown by ensure_global_ws: freed by name)
    OWN(&h->err_flag, (size_t)1);
    OWN(&h->ones_u8, (size_t)(h->H1p + h->H2p), false);
    HIPCHK(h, hipMemsetAsync(h->ones_u8, 1, (size_t)(h->H1p + h->H2p), h->st), fail());
    OWN(&h->st_ids, (size_t)h->Bmax * h->F);
    OWN(&h->st_y, (size_t)h->Bmax);
    OWN(&h->st_m1, (size_t)h->H1p); OWN(&h->st_m2, (size_t)h->H2p);
    OWN(&h->st_p, (size_t)h->Bmax);
    OWN(&h->st_x, (size_t)h->Bmax * h->xdim);
#undef OWN
    // dynamic LDS beyond the 64 KB default, set once and for every size a later call can ask for (the workspace of a global batch
    // grows monotonically, so a smaller batch after a larger one used to launch k_sort<8> without its attribute;
    // with the kernel's static counter k_sort<8> at 8192 keys is 65,540 bytes)
    HIPCHK(h, hipFuncSetAttribute((const void*)k_sort<8>, hipFuncAttributeMaxDynamicSharedMemorySize, 8192 * 8), fail());
    HIPCHK(h, hipFuncSetAttribute((const void*)k_sort<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 16384 * 8), fail());
    if (!h->bag) {
        // 65,600 bytes at F = 64, K = 15; wide rows: 133,152 at F * K = 4096, F = 64 (8 examples per tile)
        const size_t gl = (size_t)(h->wide ? GR_EX_WIDE : GR_EX) * (h->xdim + h->F) * sizeof(float);
        if (gl > 160 * 1024) FAIL(h, FNN_ERR_ARG, "n_fields * k too large for the reference-layout gather tile", fail());
        const void* kf = h->wide ? (const void*)k_gather_ref<GR_EX_WIDE, true> : (const void*)k_gather_ref<GR_EX, false>;
        HIPCHK(h, hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max(gl, (size_t)65536)), fail());
    }
    HIPCHK(h, hipStreamSynchronize(h->st), fail());
    *out = h;
    return FNN_OK;
}

int fnn_destroy(fnn_handle* h)
{
    if (!h) return FNN_ERR_ARG;
    hipSetDevice(h->dev);
    if (h->st) hipStreamSynchronize(h->st);
    if (h->comm && h->dp_own_comm && g_rccl.CommDestroy) g_rccl.CommDestroy(h->comm);
    p2p_release(h);
    for (auto& kv : h->prof_slots) for (auto& p : kv.second.ev) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    // what is regrown while the handle lives, by name; then the record of what fnn_create allocated for good
    for (void* q : {(void*)h->table16, (void*)h->field_of_row, (void*)h->tag_first, (void*)h->slot[0].tag_shared, (void*)h->slot[1].tag_shared, (void*)h->cpow_dev,
                    (void*)h->shadow_dev, (void*)h->xg_ids_send, (void*)h->xg_ids, (void*)h->xg_gxp, h->gws}) if (q) hipFree(q);
    for (void* q : h->owned) hipFree(q);
    ring_release(h->step_ring);
    ring_release(h->eval_ring);
    if (h->eval_y) hipFree(h->eval_y);
    if (h->join) hipEventDestroy(h->join);
    if (h->step_pack) hipFree(h->step_pack);
    for (fnn_handle::SortSlot* sl : {&h->slot[0], &h->slot[1], &h->gsl}) row_group_free(*sl);
    if (h->own_stream && h->st) hipStreamDestroy(h->st);
    delete h;
    return FNN_OK;
}

int fnn_set_hparams(fnn_handle* h, float lr, float lambda1, float lambda_fm)
{
    if (!h) return FNN_ERR_ARG;
    h->cfg.lr = lr; h->cfg.lambda1 = lambda1; h->cfg.lambda_fm = lambda_fm;
    return FNN_OK;
}

void* fnn_stream(fnn_handle* h) { return h ? (void*)h->st : nullptr; }

int fnn_sync(fnn_handle* h)
{
    if (!h) return FNN_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->dev));
    return check_async(h);
}

int fnn_set_table(fnn_handle* h, const float* rows, int64_t n_rows, const int32_t* field_of_row,
                  float w0, int memkind)
{
    if (!h) return FNN_ERR_ARG;
    if (!rows || n_rows <= 0 || n_rows >= (1ll << 31)) FAIL(h, FNN_ERR_ARG, "rows null or n_rows out of range");
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipStreamSynchronize(h->st));
    if (h->table16) { hipFree(h->table16); h->table16 = nullptr; }
    if (h->field_of_row) { hipFree(h->field_of_row); h->field_of_row = nullptr; }
    HIPCHK(h, hipMalloc((void**)&h->table16, (size_t)n_rows * h->rw * sizeof(float)));
    HIPCHK(h, hipMalloc((void**)&h->field_of_row, (size_t)n_rows * sizeof(int32_t)));
    const size_t nbytes = (size_t)n_rows * h->K * sizeof(float);
    const float* src = rows; float* tmp = nullptr;
    if (memkind == FNN_MEM_HOST) {
        HIPCHK(h, hipMalloc((void**)&tmp, nbytes));
        HIPCHK(h, hipMemcpy(tmp, rows, nbytes, hipMemcpyHostToDevice));
        src = tmp;
    }
    const size_t n = (size_t)n_rows * h->rw;
    hipLaunchKernelGGL(k_pack_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, src, n_rows, h->K, h->rw, h->table16);
    if (field_of_row)
        HIPCHK(h, hipMemcpyAsync(h->field_of_row, field_of_row, (size_t)n_rows * sizeof(int32_t),
                                 memkind == FNN_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->st));
    else
        HIPCHK(h, hipMemsetAsync(h->field_of_row, 0, (size_t)n_rows * sizeof(int32_t), h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    if (tmp) hipFree(tmp);
    if (h->bag) {
        for (int** q : {&h->tag_first, &h->slot[0].tag_shared, &h->slot[1].tag_shared}) {
            if (*q) { hipFree(*q); *q = nullptr; }
            HIPCHK(h, hipMalloc((void**)q, (size_t)n_rows * sizeof(int)));
            HIPCHK(h, hipMemset(*q, 0, (size_t)n_rows * sizeof(int)));
        }
        h->tag_stamp = 0;
    }
    h->n_rows = n_rows; h->w0 = w0;
    BY_PREC(h, plan_keys, (h, (unsigned long long)n_rows * SORT_N > 0xFFFFFFFFull));     // else 32-bit (row << 12 | t) keys
    h->sorted_ids = nullptr; h->next_ids = nullptr;
    return FNN_OK;
}

static int get_rows_impl(fnn_handle* h, const int64_t* row_ids, int64_t n, float* out, int memkind)
{
    if (!h->table16) FAIL(h, FNN_ERR_STATE, "fnn_set_table has not been called");
    if (!out || n <= 0) FAIL(h, FNN_ERR_ARG, "out null or n <= 0");
    HIPCHK(h, hipSetDevice(h->dev));
    const size_t cnt = (size_t)n * h->K;
    const int64_t* ids_dev = row_ids; float* out_dev = out;
    int64_t* tmp_ids = nullptr; float* tmp_out = nullptr;
    if (memkind == FNN_MEM_HOST) {
        if (row_ids) {
            HIPCHK(h, hipMalloc((void**)&tmp_ids, (size_t)n * sizeof(int64_t)));
            HIPCHK(h, hipMemcpy(tmp_ids, row_ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
            ids_dev = tmp_ids;
        }
        HIPCHK(h, hipMalloc((void**)&tmp_out, cnt * sizeof(float)));
        out_dev = tmp_out;
    }
    hipLaunchKernelGGL(k_unpack_rows, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->st, h->table16,
                       ids_dev, n, h->n_rows, h->K, h->rw, out_dev, h->err_flag);
    int rc = FNN_OK;
    if (memkind == FNN_MEM_HOST) {
        HIPCHK(h, hipMemcpyAsync(out, tmp_out, cnt * sizeof(float), hipMemcpyDeviceToHost, h->st));
        rc = check_async(h);
        if (tmp_ids) hipFree(tmp_ids);
        hipFree(tmp_out);
    }
    return rc;
}

int fnn_get_table(fnn_handle* h, float* rows_out, int memkind)
{
    if (!h) return FNN_ERR_ARG;
    return get_rows_impl(h, nullptr, h->n_rows, rows_out, memkind);
}

int fnn_get_rows(fnn_handle* h, const int64_t* row_ids, int64_t n, float* out, int memkind)
{
    if (!h) return FNN_ERR_ARG;
    if (!row_ids) FAIL(h, FNN_ERR_ARG, "row_ids null");
    return get_rows_impl(h, row_ids, n, out, memkind);
}

// Reference shapes <-> padded slot layout.  Host staging; called rarely.
int fnn_set_dense(fnn_handle* h, int layer, const float* W, const float* b, int memkind)
{
    if (!h) return FNN_ERR_ARG;
    if (layer < 1 || layer > 3 || !W || !b) FAIL(h, FNN_ERR_ARG, "layer must be 1..3, W and b non-null");
    HIPCHK(h, hipSetDevice(h->dev));
    const int F = h->F, K = h->K, H1 = h->H1, H2 = h->H2, H1p = h->H1p, H2p = h->H2p;
    const size_t nW = layer == 1 ? (size_t)h->xdim * H1 : layer == 2 ? (size_t)H1 * H2 : (size_t)H2;
    const size_t nb = layer == 1 ? H1 : layer == 2 ? H2 : 1;
    std::vector<float> hw(nW), hb(nb);
    if (memkind == FNN_MEM_HOST) { memcpy(hw.data(), W, nW * 4); memcpy(hb.data(), b, nb * 4); }
    else {
        HIPCHK(h, hipMemcpy(hw.data(), W, nW * 4, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(hb.data(), b, nb * 4, hipMemcpyDeviceToHost));
    }
    HIPCHK(h, hipStreamSynchronize(h->st));
    if (layer == 1) {
        std::vector<float> p(h->n1, 0.f);
        if (h->bag) {                                                    // W [h0][H1]; b1 on the ones column h0
            for (int i = 0; i < h->rw; ++i) memcpy(&p[(size_t)i * H1p], &hw[(size_t)i * H1], H1 * 4);
            memcpy(&p[(size_t)h->rw * H1p], hb.data(), H1 * 4);
        } else if (h->wide) {                                            // wide rows: field f at rows f*rw.., then w_0, ones
            const int rw = h->rw;
            for (int f = 0; f < F; ++f)
                for (int l = 0; l < K; ++l)
                    memcpy(&p[(size_t)(f * rw + l) * H1p], &hw[(size_t)(1 + f * K + l) * H1], H1 * 4);
            memcpy(&p[(size_t)(F * rw) * H1p], &hw[0], H1 * 4);          // w1[0,:] on the w_0 column
            memcpy(&p[(size_t)(F * rw + 1) * H1p], hb.data(), H1 * 4);   // b1 on the ones column
        } else {
            for (int f = 0; f < F; ++f)
                for (int l = 0; l < K; ++l)
                    memcpy(&p[(size_t)(f * SLOT + l) * H1p], &hw[(size_t)(1 + f * K + l) * H1], H1 * 4);
            memcpy(&p[(size_t)K * H1p], &hw[0], H1 * 4);                 // w1[0,:] rides on the w_0 slot
            memcpy(&p[(size_t)(SLOT + K) * H1p], hb.data(), H1 * 4);     // b1 rides on the ones slot
        }
        HIPCHK(h, hipMemcpy(h->master, p.data(), h->n1 * 4, hipMemcpyHostToDevice));
    } else if (layer == 2) {
        std::vector<float> p(h->n2, 0.f);
        for (int i = 0; i < H1; ++i) memcpy(&p[(size_t)i * H2p], &hw[(size_t)i * H2], H2 * 4);
        memcpy(&p[(size_t)H1 * H2p], hb.data(), H2 * 4);
        HIPCHK(h, hipMemcpy(h->master + h->n1, p.data(), h->n2 * 4, hipMemcpyHostToDevice));
    } else {
        std::vector<float> p(H2p, 0.f);
        memcpy(p.data(), hw.data(), H2 * 4); p[H2] = hb[0];
        HIPCHK(h, hipMemcpy(h->master + h->nw12, p.data(), (size_t)H2p * 4, hipMemcpyHostToDevice));
    }
    BY_PREC(h, launch_update, (h, nullptr, 0.f));
    HIPCHK(h, hipStreamSynchronize(h->st));
    h->dense_set[layer - 1] = true;
    return FNN_OK;
}

int fnn_get_dense(fnn_handle* h, int layer, float* W, float* b, int memkind)
{
    if (!h) return FNN_ERR_ARG;
    if (layer < 1 || layer > 3 || !W || !b) FAIL(h, FNN_ERR_ARG, "layer must be 1..3, W and b non-null");
    HIPCHK(h, hipSetDevice(h->dev));
    const int F = h->F, K = h->K, H1 = h->H1, H2 = h->H2, H1p = h->H1p, H2p = h->H2p;
    std::vector<float> m(h->nw);
    HIPCHK(h, hipStreamSynchronize(h->st));
    HIPCHK(h, hipMemcpy(m.data(), h->master, h->nw * 4, hipMemcpyDeviceToHost));
    const size_t nW = layer == 1 ? (size_t)h->xdim * H1 : layer == 2 ? (size_t)H1 * H2 : (size_t)H2;
    const size_t nb = layer == 1 ? H1 : layer == 2 ? H2 : 1;
    std::vector<float> hw(nW), hb(nb);
    if (layer == 1) {
        if (h->bag) {
            for (int i = 0; i < h->rw; ++i) memcpy(&hw[(size_t)i * H1], &m[(size_t)i * H1p], H1 * 4);
            memcpy(hb.data(), &m[(size_t)h->rw * H1p], H1 * 4);
        } else if (h->wide) {
            const int rw = h->rw;
            memcpy(&hw[0], &m[(size_t)(F * rw) * H1p], H1 * 4);
            for (int f = 0; f < F; ++f)
                for (int l = 0; l < K; ++l)
                    memcpy(&hw[(size_t)(1 + f * K + l) * H1], &m[(size_t)(f * rw + l) * H1p], H1 * 4);
            memcpy(hb.data(), &m[(size_t)(F * rw + 1) * H1p], H1 * 4);
        } else {
            memcpy(&hw[0], &m[(size_t)K * H1p], H1 * 4);
            for (int f = 0; f < F; ++f)
                for (int l = 0; l < K; ++l)
                    memcpy(&hw[(size_t)(1 + f * K + l) * H1], &m[(size_t)(f * SLOT + l) * H1p], H1 * 4);
            memcpy(hb.data(), &m[(size_t)(SLOT + K) * H1p], H1 * 4);
        }
    } else if (layer == 2) {
        const float* p = &m[h->n1];
        for (int i = 0; i < H1; ++i) memcpy(&hw[(size_t)i * H2], &p[(size_t)i * H2p], H2 * 4);
        memcpy(hb.data(), &p[(size_t)H1 * H2p], H2 * 4);
    } else {
        memcpy(hw.data(), &m[h->nw12], H2 * 4); hb[0] = m[h->nw12 + H2];
    }
    if (memkind == FNN_MEM_HOST) { memcpy(W, hw.data(), nW * 4); memcpy(b, hb.data(), nb * 4); }
    else {
        HIPCHK(h, hipMemcpy(W, hw.data(), nW * 4, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(b, hb.data(), nb * 4, hipMemcpyHostToDevice));
    }
    return FNN_OK;
}

int fnn_set_bag_bias(fnn_handle* h, const float* bb0, int memkind)
{
    if (!h) return FNN_ERR_ARG;
    if (!h->bag || !bb0) FAIL(h, FNN_ERR_ARG, "fnn_set_bag_bias: FNN_MODE_BAG handle and non-null pointer required");
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipStreamSynchronize(h->st));
    HIPCHK(h, hipMemcpy(h->bb0, bb0, (size_t)h->rw * 4, memkind == FNN_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
    return FNN_OK;
}

int fnn_get_bag_bias(fnn_handle* h, float* bb0_out, int memkind)
{
    if (!h) return FNN_ERR_ARG;
    if (!h->bag || !bb0_out) FAIL(h, FNN_ERR_ARG, "fnn_get_bag_bias: FNN_MODE_BAG handle and non-null pointer required");
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipStreamSynchronize(h->st));
    HIPCHK(h, hipMemcpy(bb0_out, h->bb0, (size_t)h->rw * 4, memkind == FNN_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
    return FNN_OK;
}

int fnn_gather(fnn_handle* h, const int32_t* ids, int B, float* x_out, int memkind)
{
    if (!h) return FNN_ERR_ARG;
    // any B: the reference's get_batch_data serves 100,000-line evaluation chunks (python/FNN_wnzh.py:193-221); device pointers
    // go through one launch, host pointers through the max_batch-sized staging buffers chunk by chunk
    if (B <= 0 || (size_t)B * h->xdim > (size_t)1 << 40) FAIL(h, FNN_ERR_ARG, "B must be positive");
    if (!h->table16) FAIL(h, FNN_ERR_STATE, "fnn_set_table has not been called");
    if (!ids || !x_out) FAIL(h, FNN_ERR_ARG, "null pointer");
    HIPCHK(h, hipSetDevice(h->dev));
    const bool host = memkind == FNN_MEM_HOST;
    for (int lo = 0; lo < B; lo += host ? h->Bmax : B) {
        const int nb = host ? std::min(h->Bmax, B - lo) : B;
        const int32_t* ids_dev = ids + (size_t)lo * h->F; float* x_dev = x_out + (size_t)lo * h->xdim;
        const size_t n = (size_t)nb * h->xdim;
        Staged sg{h, host};
        RCCHK(sg.in(ids_dev, h->st_ids, (size_t)nb * h->F));
        sg.out(x_dev, h->st_x, n);
        {
            ProfScope ps(h, "gather_ref", h->st);
            if (h->bag)
                hipLaunchKernelGGL(k_bag_ref, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, h->st, ids_dev, nb, h->F,
                                   h->rw, h->table16, h->n_rows, h->bb0, x_dev, h->err_flag, (h->kn.wt_stores & 16) != 0);   // (measured: 1 % slower written through -- off)
            else if (h->wide)
                hipLaunchKernelGGL((k_gather_ref<GR_EX_WIDE, true>), dim3((unsigned)((nb + GR_EX_WIDE - 1) / GR_EX_WIDE)), dim3(256), (size_t)GR_EX_WIDE * (h->xdim + h->F) * sizeof(float), h->st,
                                   ids_dev, nb, h->F, h->K, h->table16, h->n_rows, h->w0, x_dev, h->err_flag, (h->kn.wt_stores & 8) != 0, h->rw);
            else
                hipLaunchKernelGGL((k_gather_ref<GR_EX, false>), dim3((unsigned)((nb + GR_EX - 1) / GR_EX)), dim3(256), (size_t)GR_EX * (h->xdim + h->F) * sizeof(float), h->st, ids_dev, nb, h->F,
                                   h->K, h->table16, h->n_rows, h->w0, x_dev, h->err_flag, (h->kn.wt_stores & 8) != 0, SLOT);
        }
        RCCHK(sg.copy_back());
        if (host) RCCHK(check_async(h));                // (synchronises: the staging buffers are free for the next chunk)
    }
    return FNN_OK;
}

static int step_impl(fnn_handle* h, const int32_t* ids, const float* y, int B, const uint8_t* mask1,
                     const uint8_t* mask2, int b_size, float* p_out, float* gx_out, int memkind,
                     bool inline_update)
{
    RCCHK(check_ready(h, B));
    if (!ids || !y || !mask1 || !mask2) FAIL(h, FNN_ERR_ARG, "ids, y, mask1, mask2 must be non-null");
    if (h->in_step) FAIL(h, FNN_ERR_STATE, "fnn_step_begin called twice without fnn_step_end");
    HIPCHK(h, hipSetDevice(h->dev));
    if (b_size <= 0) b_size = B;
    RCCHK(update_cpow(h, b_size, B));
    Staged sg{h, memkind == FNN_MEM_HOST};
    RCCHK(sg.in(ids, h->st_ids, (size_t)B * h->F));
    RCCHK(sg.in(y, h->st_y, (size_t)B));
    RCCHK(sg.in(mask1, h->st_m1, (size_t)h->H1));
    RCCHK(sg.in(mask2, h->st_m2, (size_t)h->H2));
    sg.out(p_out, h->st_p, (size_t)B);
    sg.out(gx_out, h->st_x, (size_t)B * h->xdim);
    if (sg.host) { h->sorted_ids = nullptr; h->next_ids = nullptr; }     // staging buffers are reused: no carried grouping
    if (h->n_shadow > 0 && h->bag) FAIL(h, FNN_ERR_ARG, "fnn_set_shadowed: FNN_MODE_FM only");
    if (h->n_shadow > 0 && h->dp && inline_update && h->dp_sparse == FNN_DP_SPARSE_EXCHANGE)
        FAIL(h, FNN_ERR_ARG, "shadowed features are not carried through FNN_DP_SPARSE_EXCHANGE");
    // shadowed features: the layer-by-layer path, whose per-field sort has room for the extra keys
    const bool fast = B <= h->three_launch_max_B && h->n_shadow == 0;
    h->update_pending = !(fast && inline_update);
    h->step_native_dp = inline_update && h->dp;
    h->step_bsize = b_size;
    const int rc = fast ? BY_PREC_RC(h, run_step_fast, (h, ids, y, B, mask1, mask2, p_out, gx_out, inline_update))
                        : BY_PREC_RC(h, run_step, (h, ids, y, B, mask1, mask2, true, p_out, gx_out));
    h->n_shadow = 0;                                            // consumed (also by a failing step)
    if (rc != FNN_OK) return rc;
    RCCHK(sg.copy_back());
    if (sg.nback > 0) HIPCHK(h, hipStreamSynchronize(h->st));
    h->in_step = true; h->step_B = B;
    return FNN_OK;
}

int fnn_step_begin(fnn_handle* h, const int32_t* ids, const float* y, int B, const uint8_t* mask1,
                   const uint8_t* mask2, int b_size, float* p_out, float* gx_out, int memkind)
{
    return step_impl(h, ids, y, B, mask1, mask2, b_size, p_out, gx_out, memkind, false);
}

int fnn_set_shadowed(fnn_handle* h, const int32_t* tfr, int n, int memkind)
{
    if (!h) return FNN_ERR_ARG;
    if (n < 0 || (n > 0 && !tfr)) FAIL(h, FNN_ERR_ARG, "fnn_set_shadowed: null list or n < 0");
    if (h->bag) FAIL(h, FNN_ERR_ARG, "fnn_set_shadowed: FNN_MODE_FM only");
    if (h->in_step) FAIL(h, FNN_ERR_STATE, "fnn_set_shadowed inside a step");
    HIPCHK(h, hipSetDevice(h->dev));
    if (n > h->shadow_cap) {
        HIPCHK(h, hipStreamSynchronize(h->st));
        if (h->shadow_dev) { hipFree(h->shadow_dev); h->shadow_dev = nullptr; h->shadow_cap = 0; }
        const int cap = std::max(1024, n);
        HIPCHK(h, hipMalloc((void**)&h->shadow_dev, (size_t)cap * 3 * sizeof(int32_t)));
        h->shadow_cap = cap;
    }
    if (n > 0) {
        if (!h->table16) FAIL(h, FNN_ERR_STATE, "fnn_set_shadowed before fnn_set_table");
        HIPCHK(h, hipMemcpyAsync(h->shadow_dev, tfr, (size_t)n * 3 * sizeof(int32_t),
                                 memkind == FNN_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->st));
        // a row belongs to ONE field (fnn_set_table's field_of_row): the sparse-row update groups keys per field, so an entry that
        // names a row under another field would put the row into two groups of one launch -- two unordered read-modify-writes.
        // Checked here (a launch and a read of the flag; this call is rare), not left to show as a lost update one run in four.
        hipLaunchKernelGGL(k_check_shadowed, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->shadow_dev, n, h->field_of_row,
                           h->n_rows, h->F, h->err_flag);
        int flag = 0;
        HIPCHK(h, hipMemcpyAsync(&flag, h->err_flag, sizeof(int), hipMemcpyDeviceToHost, h->st));
        HIPCHK(h, hipStreamSynchronize(h->st));                       // (also: the caller's host buffer may go away)
        if (flag & 8) {
            HIPCHK(h, hipMemsetAsync(h->err_flag, 0, sizeof(int), h->st));
            h->n_shadow = 0;
            FAIL(h, FNN_ERR_ARG, "fnn_set_shadowed: an entry's row is outside the table or does not belong to the entry's field (field_of_row)");
        }
    }
    h->n_shadow = n;
    return FNN_OK;
}

int fnn_prefetch_ids(fnn_handle* h, const int32_t* ids, int B)
{
    RCCHK(check_ready(h, B));
    if (!ids) FAIL(h, FNN_ERR_ARG, "ids null");
    h->next_ids = ids; h->next_B = B;       // grouped by the next step's first launch
    return FNN_OK;
}

int fnn_step_scatter(fnn_handle* h)
{
    if (!h) return FNN_ERR_ARG;
    if (!h->in_step) FAIL(h, FNN_ERR_STATE, "fnn_step_scatter without fnn_step_begin");
    HIPCHK(h, hipSetDevice(h->dev));
    if (h->scatter_pending) {
        BY_PREC(h, launch_steps23, (h, make_roles(h, false, true, false)));
        HIPCHK(h, hipGetLastError());
    }
    return FNN_OK;
}

int fnn_sparse_grad(fnn_handle* h, float** dev_ptr, int64_t* row_floats)
{
    if (!h || !dev_ptr || !row_floats) return FNN_ERR_ARG;
    if (h->bag) FAIL(h, FNN_ERR_ARG, "fnn_sparse_grad: FNN_MODE_FM only");
    if (h->wide) FAIL(h, FNN_ERR_ARG, "fnn_sparse_grad: the 16-float slot layout of the exact data-parallel mode; not supported on wide rows (k >= 17)");
    *dev_ptr = h->gxp; *row_floats = h->K1p;
    return FNN_OK;
}

int fnn_step_scatter_global(fnn_handle* h, const int32_t* ids_g, const float* gxp_g, int B_g)
{
    if (!h) return FNN_ERR_ARG;
    if (h->wide) FAIL(h, FNN_ERR_ARG, "fnn_step_scatter_global: the 16-float slot layout of the exact data-parallel mode; not supported on wide rows (k >= 17)");
    if (!h->in_step) FAIL(h, FNN_ERR_STATE, "fnn_step_scatter_global without fnn_step_begin");
    if (h->bag) FAIL(h, FNN_ERR_ARG, "fnn_step_scatter_global: FNN_MODE_FM only");
    if (!ids_g || !gxp_g || B_g < 1 || B_g > GLOBAL_BATCH_MAX) FAIL(h, FNN_ERR_ARG, "ids_g / gxp_g null or B_g outside [1, 32768]");
    HIPCHK(h, hipSetDevice(h->dev));
    return scatter_global_impl(h, ids_g, gxp_g, B_g);
}

int fnn_dp_unique_id(void* id128_out)
{
    if (!id128_out) { g_create_err = "fnn_dp_unique_id: null pointer"; return FNN_ERR_ARG; }
    RCCHK(rccl_load(g_create_err));
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    const ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) { g_create_err = std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r); return FNN_ERR_HIP; }
    memcpy(id128_out, &id, sizeof(id));
    return FNN_OK;
}

int fnn_dp_shutdown(fnn_handle* h)
{
    if (!h) return FNN_ERR_ARG;
    if (h->in_step) FAIL(h, FNN_ERR_STATE, "fnn_dp_shutdown inside a step");
    hipSetDevice(h->dev);
    if (h->st) hipStreamSynchronize(h->st);
    if (h->comm && h->dp_own_comm && g_rccl.CommDestroy) g_rccl.CommDestroy(h->comm);
    h->comm = nullptr; h->dp_own_comm = false;
    h->dp = false; h->dp_allreduce = nullptr; h->dp_allgather = nullptr; h->dp_ctx = nullptr;
    h->dp_rank = 0; h->dp_world = 1; h->dp_sparse = FNN_DP_SPARSE_LOCAL;
    p2p_release(h);
    h->dp_payload = FNN_DP_PAYLOAD_SLABS; h->dp_collective = FNN_DP_COLLECTIVE_CALLBACK;
    return FNN_OK;
}

int fnn_dp_set_payload(fnn_handle* h, int payload)
{
    if (!h) return FNN_ERR_ARG;
    if (payload != FNN_DP_PAYLOAD_SLABS && payload != FNN_DP_PAYLOAD_BUCKET) FAIL(h, FNN_ERR_ARG, "fnn_dp_set_payload: bad payload");
    if (h->in_step) FAIL(h, FNN_ERR_STATE, "fnn_dp_set_payload inside a step");
    h->dp_payload = payload;
    return FNN_OK;
}

int fnn_dp_p2p_export(fnn_handle* h, void* handle64_out, int same_process)
{
    if (!h || !handle64_out) return FNN_ERR_ARG;
    if (!h->dp) FAIL(h, FNN_ERR_STATE, "fnn_dp_p2p_export before fnn_dp_init / fnn_dp_init_custom");
    if (h->dp_world > 8) FAIL(h, FNN_ERR_ARG, "the p2p all-reduce serves up to 8 ranks (one node)");
    if (h->in_step) FAIL(h, FNN_ERR_STATE, "fnn_dp_p2p_export inside a step");
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipStreamSynchronize(h->st));
    p2p_release(h);
    h->xr_nbp = (size_t)rup((int)(h->nw + h->nbag), 64);
    h->xr_bytes = 2 * h->xr_nbp * sizeof(float) + 8 * 64;
    // memory that stays coherent between devices: uncached, else fine-grained ($FNN_P2P_REGION = uncached | finegrained | plain
    // picks one; plain hipMalloc only where the ranks share a process and a device)
    const char* want = getenv("FNN_P2P_REGION");
    void* q = nullptr; h->xr_kind = 0;
    if ((!want || !strcmp(want, "uncached")) && hipExtMallocWithFlags(&q, h->xr_bytes, hipDeviceMallocUncached) == hipSuccess) h->xr_kind = 1;
    else if ((!want || !strcmp(want, "finegrained")) && hipExtMallocWithFlags(&q, h->xr_bytes, hipDeviceMallocFinegrained) == hipSuccess) h->xr_kind = 2;
    else if (((!want && same_process) || (want && !strcmp(want, "plain"))) && hipMalloc(&q, h->xr_bytes) == hipSuccess) h->xr_kind = 3;
    (void)hipGetLastError();
    if (!h->xr_kind) FAIL(h, FNN_ERR_NOMEM, "fnn_dp_p2p_export: no uncached / fine-grained device memory for the exchange region");
    h->xr = static_cast<float*>(q);
    HIPCHK(h, hipMemset(h->xr, 0, h->xr_bytes));
    if (!h->p2p_wait_max) HIPCHK(h, hipMalloc((void**)&h->p2p_wait_max, 8));
    HIPCHK(h, hipMemset(h->p2p_wait_max, 0, 8));
    if (const char* ev2 = getenv("FNN_P2P_TIMEOUT_MS")) { const long long ms = atoll(ev2); if (ms > 0) h->p2p_timeout_ticks = (unsigned long long)ms * 100000ull; }
    h->xr_same_process = same_process != 0;
    memset(handle64_out, 0, 64);
    if (same_process) memcpy(handle64_out, &h->xr, sizeof(void*));
    else {
        static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
        hipIpcMemHandle_t mh;
        HIPCHK(h, hipIpcGetMemHandle(&mh, h->xr));
        memcpy(handle64_out, &mh, 64);
    }
    return FNN_OK;
}

int fnn_dp_p2p_attach(fnn_handle* h, const void* handles, int same_process)
{
    if (!h || !handles) return FNN_ERR_ARG;
    if (!h->dp || !h->xr) FAIL(h, FNN_ERR_STATE, "fnn_dp_p2p_attach before fnn_dp_p2p_export");
    if ((same_process != 0) != h->xr_same_process) FAIL(h, FNN_ERR_ARG, "fnn_dp_p2p_attach: same_process differs from fnn_dp_p2p_export");
    HIPCHK(h, hipSetDevice(h->dev));
    const char* hs = static_cast<const char*>(handles);
    for (int r = 0; r < h->dp_world; ++r) {
        if (r == h->dp_rank) { h->peer[r] = h->xr; continue; }
        if (same_process) { void* q; memcpy(&q, hs + 64 * r, sizeof(void*)); h->peer[r] = static_cast<float*>(q); continue; }
        hipIpcMemHandle_t mh; memcpy(&mh, hs + 64 * r, 64);
        void* q = nullptr;
        HIPCHK(h, hipIpcOpenMemHandle(&q, mh, hipIpcMemLazyEnablePeerAccess));
        h->peer[r] = static_cast<float*>(q); h->peer_opened[r] = true;
    }
    for (int r = 0; r < h->dp_world; ++r) if (!h->peer[r]) FAIL(h, FNN_ERR_ARG, "fnn_dp_p2p_attach: a null region");
    h->p2p_attached = true; h->dp_step_no = 0;
    return FNN_OK;
}

int fnn_dp_set_collective(fnn_handle* h, int collective)
{
    if (!h) return FNN_ERR_ARG;
    if (collective != FNN_DP_COLLECTIVE_CALLBACK && collective != FNN_DP_COLLECTIVE_P2P) FAIL(h, FNN_ERR_ARG, "fnn_dp_set_collective: bad collective");
    if (h->in_step) FAIL(h, FNN_ERR_STATE, "fnn_dp_set_collective inside a step");
    if (collective == FNN_DP_COLLECTIVE_P2P && !(h->dp && h->p2p_attached)) FAIL(h, FNN_ERR_STATE, "FNN_DP_COLLECTIVE_P2P needs fnn_dp_p2p_export + fnn_dp_p2p_attach on every rank first");
    h->dp_collective = collective;
    return FNN_OK;
}

int fnn_dp_p2p_max_wait_us(fnn_handle* h, double* us_out)
{
    if (!h || !us_out) return FNN_ERR_ARG;
    *us_out = 0.0;
    if (!h->p2p_wait_max) return FNN_OK;
    HIPCHK(h, hipSetDevice(h->dev));
    unsigned long long t = 0;
    HIPCHK(h, hipMemcpyAsync(&t, h->p2p_wait_max, 8, hipMemcpyDeviceToHost, h->st));
    HIPCHK(h, hipStreamSynchronize(h->st));
    *us_out = (double)t / 100.0;
    return FNN_OK;
}

int fnn_dp_get_config(fnn_handle* h, int* payload, int* collective, int* region_kind)
{
    if (!h) return FNN_ERR_ARG;
    if (payload) *payload = dp_bucket_mode(h) ? FNN_DP_PAYLOAD_BUCKET : FNN_DP_PAYLOAD_SLABS;
    if (collective) *collective = h->dp_collective;
    if (region_kind) *region_kind = h->xr_kind;
    return FNN_OK;
}

int fnn_dp_init(fnn_handle* h, int rank, int world, const void* id128, int sparse_mode)
{
    if (!h) return FNN_ERR_ARG;
    if (!id128) FAIL(h, FNN_ERR_ARG, "fnn_dp_init: null unique id");
    if (h->dp) RCCHK(fnn_dp_shutdown(h));
    HIPCHK(h, hipSetDevice(h->dev));
    RCCHK(rccl_load(h->err));
    RCCHK(dp_setup(h, rank, world, sparse_mode));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    HIPCHK(h, hipStreamSynchronize(h->st));
    const ncclResult_t r = g_rccl.CommInitRank(&h->comm, world, id, rank);
    if (r != ncclSuccess) { h->comm = nullptr; FAIL(h, FNN_ERR_HIP, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r)); }
    h->dp_own_comm = true;
    h->dp_allreduce = rccl_allreduce_cb; h->dp_allgather = rccl_allgather_cb; h->dp_ctx = h;
    h->dp = true;
    return FNN_OK;
}

int fnn_dp_init_custom(fnn_handle* h, int rank, int world, fnn_allreduce_fn allreduce, fnn_allgather_fn allgather, void* ctx,
                       int sparse_mode)
{
    if (!h) return FNN_ERR_ARG;
    if (!allreduce || (sparse_mode == FNN_DP_SPARSE_EXCHANGE && !allgather)) FAIL(h, FNN_ERR_ARG, "fnn_dp_init_custom: null callback");
    if (h->dp) RCCHK(fnn_dp_shutdown(h));
    HIPCHK(h, hipSetDevice(h->dev));
    RCCHK(dp_setup(h, rank, world, sparse_mode));
    h->dp_allreduce = allreduce; h->dp_allgather = allgather; h->dp_ctx = ctx;
    h->dp = true;
    return FNN_OK;
}

int fnn_dense_grad_bucket(fnn_handle* h, float** dev_ptr, int64_t* n_floats)
{
    if (!h || !dev_ptr || !n_floats) return FNN_ERR_ARG;
    *dev_ptr = h->bucket; *n_floats = (int64_t)(h->nw + h->nbag);
    return FNN_OK;
}

int fnn_step_end(fnn_handle* h, float* loss_sum_out)
{
    if (!h) return FNN_ERR_ARG;
    if (!h->in_step) FAIL(h, FNN_ERR_STATE, "fnn_step_end without fnn_step_begin");
    HIPCHK(h, hipSetDevice(h->dev));
    if (h->scatter_pending) RCCHK(fnn_step_scatter(h));
    if (h->update_pending) {
        if (h->step_native_dp && dp_bucket_mode(h)) {     // layer-by-layer path under native data parallelism, bucket payload
            RCCHK(BY_PREC_RC(h, dp_finish_bucket, (h, false)), h->in_step = false);
        } else {                                           // (slabs payload: k_reduce already summed GLOBAL slabs)
            ProfScope ps(h, "update", h->st);
            BY_PREC(h, launch_update, (h, h->bucket, h->cfg.lr));
        }
    }
    HIPCHK(h, hipGetLastError());
    h->in_step = false;
    if (loss_sum_out) return fnn_last_loss(h, loss_sum_out);
    return FNN_OK;
}

int fnn_last_loss(fnn_handle* h, float* loss_sum_out)
{
    if (!h || !loss_sum_out) return FNN_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipMemcpyAsync(loss_sum_out, h->loss_dev, sizeof(float), hipMemcpyDeviceToHost, h->st));
    return check_async(h);
}

int fnn_train_step(fnn_handle* h, const int32_t* ids, const float* y, int B, const uint8_t* mask1,
                   const uint8_t* mask2, int b_size, float* p_out, float* gx_out, int memkind,
                   float* loss_sum_out)
{
    RCCHK(step_impl(h, ids, y, B, mask1, mask2, b_size, p_out, gx_out, memkind, true));
    return fnn_step_end(h, loss_sum_out);
}

// One step of several handles on one feed: per launch class the three launches of run_step_fast with the model as a grid
// dimension ("The FNN step for many models" and "The SNN fine-tune step for many models").  One body for
// both families: `bag` says which one the entry point `name` takes, FNN_MODE_FM handles or FNN_MODE_BAG handles.
static int train_step_group(const char* name, const bool bag, fnn_handle* const* hs, int n_models, const int32_t* ids, const float* y, int B,
                            const uint8_t* const* mask1, const uint8_t* const* mask2, int b_size,
                            const int32_t* next_ids, int next_B, float* const* p_out, float* loss_sum_out)
{
    FnnGroup g(name, hs, n_models, FNN_STEP_MAX_MODELS, g_create_err);
    const int M = n_models;
    // ---- refusals: all of them before anything is launched or written
    RCCHK(g.check_list("two updates would race on one model"));
    fnn_handle* h0 = g.h0;
    if (!ids || !y || !mask1 || !mask2) return g.refuse(FNN_ERR_ARG, "null ids, y, mask1 or mask2");
    for (int m = 0; m < M; ++m) if (!mask1[m] || !mask2[m]) return g.refuse(FNN_ERR_ARG, g.at("null mask1 or mask2", m));
    if (B < 1 || B > SORT_N) return g.refuse(FNN_ERR_ARG, "B must be in [1, 4096]");
    for (int m = 0; m < M; ++m) if (B > hs[m]->Bmax) return g.refuse(FNN_ERR_ARG, g.at("B must be in [1, max_batch]", m));
    if (next_ids && (next_B < 1 || next_B > SORT_N)) return g.refuse(FNN_ERR_ARG, "next_B must be in [1, 4096]");
    for (int m = 0; m < M; ++m) {
        const fnn_handle* h = hs[m];
        if (next_ids && next_B > h->Bmax) return g.refuse(FNN_ERR_ARG, g.at("next_B must be in [1, max_batch]", m));
        if (h->bag != bag) return g.refuse(FNN_ERR_ARG, g.at(bag ? "FNN_MODE_FM handles take fnn_train_step_multi" : "FNN_MODE_BAG handles take fnn_train_step, one at a time", m));
        if (h->wide) return g.refuse(FNN_ERR_ARG, g.at("wide rows (k >= 17) take fnn_train_step, one at a time", m));
        if (!h->strip_ok) return g.refuse(FNN_ERR_ARG, g.at("the handle does not run the strip kernel (hidden sizes it is not built for, or FNN_NO_FUSE=1)", m));
        if (h->n_shadow > 0) return g.refuse(FNN_ERR_ARG, g.at("shadowed features pending (fnn_set_shadowed): such a batch takes fnn_train_step", m));
        if (h->dp) return g.refuse(FNN_ERR_ARG, g.at("a data-parallel handle (fnn_dp_init) takes fnn_train_step", m));
    }
    for (int m = 0; m < M; ++m) {
        const fnn_handle* h = hs[m];
        if (!h->table16) return g.refuse(FNN_ERR_STATE, g.at("fnn_set_table has not been called", m));
        if (!(h->dense_set[0] && h->dense_set[1] && h->dense_set[2])) return g.refuse(FNN_ERR_STATE, g.at("fnn_set_dense has not been called for all three layers", m));
        if (h->in_step) return g.refuse(FNN_ERR_STATE, g.at("inside fnn_step_begin / fnn_step_end", m));
    }
    if (b_size <= 0) b_size = B;
    if (M == 1) {              // nothing to share: the solo step itself, without the argument copy
        if (next_ids) RCCHK(fnn_prefetch_ids(h0, next_ids, next_B));
        const int rs = fnn_train_step(h0, ids, y, B, mask1[0], mask2[0], b_size, p_out ? p_out[0] : nullptr, nullptr, FNN_MEM_DEVICE, loss_sum_out);
        if (rs == FNN_ERR_RANGE) g.refuse(rs, "feature id outside [-1, n_rows) in model(s) 0");
        return rs;
    }

    RCCHK(g.enter());
    const hipStream_t st = h0->st;
    // per-model preparation that copies to the device, inside the scope: the decay table when lr, lambda_fm or b_size changed
    for (int m = 0; m < M; ++m) {
        fnn_handle* h = hs[m];
        const int rc = on_stream(h, st, [&] { return update_cpow(h, b_size, B); });
        if (rc != FNN_OK) return g.member_failed(rc, h, m);
    }
    // launch classes, in the order of their first members
    std::vector<LaunchClass> cls;
    for (int m = 0; m < M; ++m) {
        LaunchClass c = BY_PREC_RC(hs[m], launch_class_of, (hs[m]));
        cls[class_index(cls, c)].members.push_back(m);
    }
    size_t slot = 0;
    HIPCHK(h0, ring_take(h0->step_ring, (size_t)M, &slot));
    char* a = h0->step_ring.host_bytes(slot);
    const char* d = h0->step_ring.dev_bytes(slot);
    if (loss_sum_out && !h0->step_pack) HIPCHK(h0, hipMalloc((void**)&h0->step_pack, FNN_STEP_MAX_MODELS * sizeof(GroupPack)));
    GroupPack* pack = loss_sum_out ? h0->step_pack : nullptr;

    struct Launch { const void* dev; int nmlp, x2, x3; };
    std::vector<Launch> launches;
    std::vector<char> have_next(M, 0);                                // per member: the next batch's grouping rides in its sort roles
    size_t pos = 0;
    for (LaunchClass& c : cls) {
        // grouping classes: the members of equal n_rows share the grouping of the first of them
        std::vector<fnn_handle*> lead(c.members.size());
        for (size_t i = 0; i < c.members.size(); ++i) {
            size_t j = 0;
            while (hs[c.members[j]]->n_rows != hs[c.members[i]]->n_rows) ++j;
            lead[i] = hs[c.members[j]];
        }
        Launch L{d + pos * h0->step_ring.elem, 0, 0, 0};
        for (size_t i = 0; i < c.members.size(); ++i) {
            const int m = c.members[i];
            fnn_handle* h = hs[m];
            h->pend_Ba = rup(B, 256);
            h->update_pending = false; h->step_native_dp = false; h->step_bsize = b_size; h->step_B = B;
            if (h == lead[i]) {
                // grouping of THIS batch: done by the previous call (next_ids) or right now, as in run_step_fast
                if (!(h->sorted_ids == ids && h->sorted_B == B)) {
                    h->prefetch_misses++;
                    fnn_handle::SortSlot& sl = h->slot[h->cur];
                    // (bag mode draws the slot's stamp, as run_step_fast does; on FM rows there are no marks and the stamp is 0)
                    on_stream(h, st, [&] { launch_sort16(h, SortArgs{ids, B, h->F, h->n_rows, sl.rec, sl.owner_cnt, h->F, h->skeys, h->tag_first, sl.tag_shared, next_stamp(h, sl)}); return 0; });
                    h->sorted_ids = ids; h->sorted_B = B;             // what the slot holds from here on, whatever becomes of the call
                } else h->prefetch_hits++;
                if (next_ids) { h->next_ids = next_ids; h->next_B = next_B; }
                h->pend_have_next = h->next_ids != nullptr && !(h->next_ids == ids && h->next_B == B);
            } else {
                h->next_ids = nullptr; h->next_B = 0; h->pend_have_next = false;
            }
            // (the first member comes before its followers: its slot holds the batch's grouping, stamp included, by now; the stamp of
            // the NEXT batch's grouping is drawn on the group's stream too)
            int x2 = 0, x3 = 0;
            const fnn_handle::SortSlot& grp = lead[i]->slot[lead[i]->cur];
            have_next[m] = on_stream(h, st, [&] { return BY_PREC_RC(h, fill_group_arg, (h, grp, ids, y, B, mask1[m], mask2[m], p_out ? p_out[m] : nullptr,
                                                                 pack ? pack + m : nullptr, a + (pos + i) * h0->step_ring.elem, &x2, &x3)); });
            L.nmlp = h->pend_Ba / 16; L.x2 = std::max(L.x2, x2); L.x3 = std::max(L.x3, x3);
        }
        launches.push_back(L);
        pos += c.members.size();
    }
    HIPCHK(h0, hipGetLastError());
    HIPCHK(h0, ring_send(h0->step_ring, slot, (size_t)M, st));
    for (size_t i = 0; i < cls.size(); ++i) {
        const Launch& L = launches[i];
        BY_PREC(hs[cls[i].members[0]], launch_group, (cls[i], st, L.dev, L.nmlp, L.x2, L.x3));
    }
    HIPCHK(h0, hipGetLastError());
    // the step is enqueued: only now the members' bookkeeping says so (the first members' slots flip, the others keep no grouping)
    for (int m = 0; m < M; ++m) sparse_role_done(hs[m], have_next[m] != 0);
    RCCHK(g.leave());
    if (!loss_sum_out) return FNN_OK;
    std::vector<GroupPack> hp(M);
    HIPCHK(h0, hipMemcpyAsync(hp.data(), pack, (size_t)M * sizeof(GroupPack), hipMemcpyDeviceToHost, st));
    HIPCHK(h0, hipStreamSynchronize(st));
    std::string bad;
    for (int m = 0; m < M; ++m) {
        loss_sum_out[m] = hp[m].loss;
        if (hp[m].flag) {
            eval_list_add(bad, m);
            HIPCHK(h0, hipMemsetAsync(hs[m]->err_flag, 0, sizeof(int), st));
        }
    }
    if (!bad.empty()) {
        HIPCHK(h0, hipStreamSynchronize(st));
        return g.refuse(FNN_ERR_RANGE, "feature id outside [-1, n_rows) in model(s) " + bad);
    }
    return FNN_OK;
}

int fnn_train_step_multi(fnn_handle* const* hs, int n_models, const int32_t* ids, const float* y, int B,
                         const uint8_t* const* mask1, const uint8_t* const* mask2, int b_size,
                         const int32_t* next_ids, int next_B, float* const* p_out, float* loss_sum_out)
{
    return train_step_group("fnn_train_step_multi", false, hs, n_models, ids, y, B, mask1, mask2, b_size, next_ids, next_B, p_out, loss_sum_out);
}

int fnn_bag_train_step_multi(fnn_handle* const* hs, int n_models, const int32_t* ids, const float* y, int B,
                             const uint8_t* const* mask1, const uint8_t* const* mask2, int b_size,
                             const int32_t* next_ids, int next_B, float* const* p_out, float* loss_sum_out)
{
    return train_step_group("fnn_bag_train_step_multi", true, hs, n_models, ids, y, B, mask1, mask2, b_size, next_ids, next_B, p_out, loss_sum_out);
}

int fnn_predict(fnn_handle* h, const int32_t* ids, int B, float* p_out, int memkind)
{
    RCCHK(check_ready(h, B));
    if (!ids || !p_out) FAIL(h, FNN_ERR_ARG, "null pointer");
    HIPCHK(h, hipSetDevice(h->dev));
    Staged sg{h, memkind == FNN_MEM_HOST};
    RCCHK(sg.in(ids, h->st_ids, (size_t)B * h->F));
    sg.out(p_out, h->st_p, (size_t)B);
    RCCHK(BY_PREC_RC(h, run_step, (h, ids, nullptr, B, nullptr, nullptr, false, p_out, nullptr)));
    HIPCHK(h, hipGetLastError());
    RCCHK(sg.copy_back());
    return sg.host ? check_async(h) : FNN_OK;
}

int fnn_eval(fnn_handle* h, const int32_t* ids, const int32_t* y, int64_t N, int memkind, double* auc, double* rmse,
             double* logloss, float* p_out)
{
    RCCHK(check_ready(h, 1));
    if (!ids || !y || N < 1) FAIL(h, FNN_ERR_ARG, "ids / y null or N < 1");
    HIPCHK(h, hipSetDevice(h->dev));
    const bool host = memkind == FNN_MEM_HOST;
    int32_t *ids_d = nullptr, *y_d = nullptr; float* p_d = nullptr;
    auto cleanup = [&]() { if (host) { if (ids_d) hipFree(ids_d); if (y_d) hipFree(y_d); } if (p_d && p_d != p_out) hipFree(p_d); };
    if (host) {
        HIPCHK(h, hipMalloc((void**)&ids_d, (size_t)N * h->F * 4), cleanup()); HIPCHK(h, hipMalloc((void**)&y_d, (size_t)N * 4), cleanup());
        HIPCHK(h, hipMemcpyAsync(ids_d, ids, (size_t)N * h->F * 4, hipMemcpyHostToDevice, h->st), cleanup());
        HIPCHK(h, hipMemcpyAsync(y_d, y, (size_t)N * 4, hipMemcpyHostToDevice, h->st), cleanup());
    } else { ids_d = const_cast<int32_t*>(ids); y_d = const_cast<int32_t*>(y); }
    if (p_out && !host) p_d = p_out; else HIPCHK(h, hipMalloc((void**)&p_d, (size_t)N * 4), cleanup());
    for (int64_t lo = 0; lo < N; lo += h->Bmax) {
        const int B = (int)std::min<int64_t>(h->Bmax, N - lo);
        RCCHK(BY_PREC_RC(h, run_step, (h, ids_d + lo * h->F, nullptr, B, nullptr, nullptr, false, p_d + lo, nullptr)), cleanup());
    }
    HIPCHK(h, hipGetLastError(), cleanup());
    double out[4] = {0, 0, 0, 0};
    std::string merr;
    const int mrc = device_metrics(h->st, p_d, y_d, N, out, merr);
    if (mrc == -1) FAIL(h, FNN_ERR_HIP, merr, cleanup());
    if (p_out && host) HIPCHK(h, hipMemcpy(p_out, p_d, (size_t)N * 4, hipMemcpyDeviceToHost), cleanup());
    cleanup();
    if (auc) *auc = out[0];
    if (rmse) *rmse = out[1];
    if (logloss) *logloss = out[2];
    RCCHK(check_async(h));
    if (mrc == -2 || mrc == -3) FAIL(h, FNN_ERR_RANGE, merr);
    return FNN_OK;
}

// The predictions of several handles on one feed: per prediction launch class ONE launch with the model as a grid dimension
// ("Evaluating many FNN models").  Nothing is allocated after hs[0]'s first group call, nothing synchronises.
int fnn_predict_multi(fnn_handle* const* hs, int n_models, const int32_t* ids, int64_t N, float* const* p_out)
{
    FnnGroup g("fnn_predict_multi", hs, n_models, FNN_EVAL_MAX_MODELS, g_create_err);
    RCCHK(pred_check(g, ids, false, nullptr, N, true, p_out));
    const EvalKnobs ek = read_eval_knobs();
    RCCHK(g.enter());
    RCCHK(ensure_eval_y(g.h0));
    const GroupPredArg<float>* d = nullptr;
    RCCHK(pred_forward(g, hs, n_models, 0, ids, N, p_out, ek, &d));
    return g.leave();
}

// ... and their metrics: the models in groups of as many as fit the scratch cap, per group the predictions, metrics_multi on
// them, the range flags, one copy home and one synchronisation.
int fnn_eval_multi(fnn_handle* const* hs, int n_models, const int32_t* ids, const int32_t* y, int64_t N,
                   double* auc, double* rmse, double* logloss, int* status, float* const* p_out)
{
    FnnGroup g("fnn_eval_multi", hs, n_models, FNN_EVAL_MAX_MODELS, g_create_err);
    RCCHK(pred_check(g, ids, true, y, N, false, nullptr));
    fnn_handle* h0 = g.h0;
    const EvalKnobs ek = read_eval_knobs();
    const int G = eval_group_size(n_models, N, "FNN_EVAL_SCRATCH_BYTES");
    RCCHK(g.enter());
    RCCHK(ensure_eval_y(h0));
    const hipStream_t st = h0->st;
    char* scratch = nullptr;                                          // the call's own
    HIPCHK(h0, hipMalloc((void**)&scratch, EvalScratch::bytes(G, N)));
    const GroupPredArg<float>* d = nullptr;                           // the group's arguments on the device, from its forward to its flags
    const EvalForward forward = [&](int g0, int n, float* const* p) { return pred_forward(g, hs + g0, n, g0, ids, N, p, ek, &d); };
    const EvalFlags flags = [&](int, int n, int* flags_d) {
        hipLaunchKernelGGL(k_gpred_flags, dim3(1), dim3(256), 0, st, d, n, flags_d);
        HIPCHK(h0, hipGetLastError());
        return FNN_OK;
    };
    EvalFound found;
    const int rc = eval_groups(st, n_models, G, y, N, scratch, forward, flags, EvalOut{auc, rmse, logloss, status, p_out}, found, h0->err);
    const int rj = g.leave();
    hipFree(scratch);                                                 // (after an error eval_groups has drained the stream)
    if (rc != FNN_OK) return rc;
    if (rj != FNN_OK) return rj;
    const std::string msg = eval_verdict(found.bad, found.range, found.n_pos, N, "[-1, n_rows)");
    return msg.empty() ? FNN_OK : g.refuse(FNN_ERR_RANGE, msg);
}

int fnn_prof_enable(fnn_handle* h, int on) { if (!h) return FNN_ERR_ARG; h->prof = on != 0; return FNN_OK; }

static int prof_collect(fnn_handle* h)
{
    HIPCHK(h, hipStreamSynchronize(h->st));
    for (auto& kv : h->prof_slots) {
        for (auto& p : kv.second.ev) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) { kv.second.ms += ms; kv.second.n += 1; }
            hipEventDestroy(p.first); hipEventDestroy(p.second);
        }
        kv.second.ev.clear();
    }
    return FNN_OK;
}

int fnn_prof_reset(fnn_handle* h)
{
    if (!h) return FNN_ERR_ARG;
    int rc = prof_collect(h);
    h->prof_slots.clear();
    return rc;
}

int fnn_prof_get(fnn_handle* h, const char* which, double* avg_ms, int64_t* launches)
{
    if (!h || !which || !avg_ms) return FNN_ERR_ARG;
    RCCHK(prof_collect(h));
    auto it = h->prof_slots.find(which);
    if (it == h->prof_slots.end() || it->second.n == 0) { *avg_ms = 0.0; if (launches) *launches = 0; return FNN_OK; }
    *avg_ms = it->second.ms / (double)it->second.n;
    if (launches) *launches = it->second.n;
    return FNN_OK;
}

}  // extern "C"
