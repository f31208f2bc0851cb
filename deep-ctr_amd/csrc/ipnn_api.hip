// ipnn_api.hip -- the inner-product FNN family (FNN_IP_L3 / L5 / L7) on gfx950: the host side and the C ABI
// (include/ipnn_hip.h).  Replaces the TensorFlow graph of python/FNN_IP_L7.py:102-133 (forward),
// :82-88 (loss) and its gradient step (plain SGD).  Built from the FNN path's pieces: the
// fragment-tiled MFMA GEMM with fused epilogues (k_gemm_ft: forward, backward-data and the split-K
// weight-gradient product of every layer, 64 x 64 per wave, operands double-buffered in registers) and the
// sorted, atomics-free sparse-row update (k_sortA / k_sortB / k_scat1 / k_scat2) -- plus the family's own kernels,
// which this unit alone includes: the inner-product layer (ip_gather_kernels.hip.h), the strip kernels of the deep
// stack (ip_strip_kernels.hip.h), the masks and updates of a step (ip_step_kernels.hip.h) and the group forms of the
// calls on many models (ip_group_kernels.hip.h).  Here: the handle, the knobs, the step plan, the kernel selectors,
// one call (ip_run), the group calls and the C ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/fnn_hip.h"
#include "../../include/ipnn_hip.h"
#include "arg_ring.h"
#include "group_call.h"
#include "fnn_kernels.hip.h"
#include "sparse_rows.hip.h"
#include "metrics.hip.h"
#include "optim.hip.h"
#include "ip_gather_kernels.hip.h"
#include "ip_strip_kernels.hip.h"
#include "ip_step_kernels.hip.h"
#include "ip_group_kernels.hip.h"

using namespace fnn;

namespace {

thread_local std::string g_ip_err;
inline int rup(int x, int m) { return (x + m - 1) / m * m; }

// The A/B knobs of a handle, read from the environment ONCE, by ip_read_knobs in ipnn_create: a variable changed while a handle
// lives does nothing to it.  The forms measured slower stay: the tests hold the forms against each other through these knobs.
struct IpKnobs {
    int side_stream = 1;                             // IPNN_SIDE_STREAM=0: everything in line on the handle's stream
    int upd_side = 0;                                // IPNN_UPDATE_SIDE=1: the dense update at the end of the side chain (ip_run; measured slower)
    int mask_side = 0;                               // IPNN_MASK_SIDE=1: the mask transposition on the side stream
    int strip = 1;                                   // IPNN_STRIP=0: one GEMM launch per product instead of the strip kernels
    int strip_l0 = 1;                                // IPNN_STRIP_L0=0: no strips for a layer 0 wider than 1024 columns (two equal tiles only: ip_strip_plan)
    int gemm_lds = 0;                                // IPNN_GEMM_LDS=1: LDS-staged k_gemm_lds for the wide products (measured equal to k_gemm_ft: both L2-bound)
    int duo = 1, duo_min = DUO_MIN_BLOCKS;           // IPNN_STRIP_DUO=0: one workgroup per strip (StripDuo); IPNN_DUO_MIN: narrowest product a pair splits
    int tail_split = 1;                              // IPNN_TAIL_SPLIT=0: the whole stack in one strip launch per direction (round 2's form)
    int tail_fuse = 1;                               // IPNN_TAIL_FUSE: training steps run the forward and the backward tail in one launch
    int tail_nf = 1, tail_nw = 16;                   // IPNN_TAIL_NF (1 / 2 / 4), IPNN_TAIL_NW (8 / 16): fragments per item and waves of the 16-example tail strips
    int tail_w_lds = 0;                              // IPNN_TAIL_LDS=1: the tail's small weights in LDS behind the tiles (ip_tail_weights; measured slower)
    int wide_nf = 2, wide_nw = 8;                    // IPNN_WIDE=nf:nw -- items (16-column fragments) and waves of the wide (pair) launches: 2:8, 4:8, 2:12
    int strip_rot = 1, fwd_skip = 0;                 // IPNN_STRIP_ROT (0: every workgroup walks the blocks in the same order), IPNN_FWD_SKIP (diagnostics)
    int strip_warm = 1;                              // IPNN_STRIP_WARM: the strip kernels touch their argument lines at the start (strip_warm_args)
    int ipf_nt = 1024;                               // IPNN_IPF_NT: threads per workgroup of the gather + inner-product launch (512 / 1024)
    bool wt = true;                                  // IPNN_WT=0: plain stores where the launches write through by default
    int group_wgrad = 1, group_xcd = 1;              // IPNN_GROUP_WGRAD=0: one launch per weight-gradient product; IPNN_GROUP_XCD=0: tiles in launch order
    int wgrad_want = 0;                              // IPNN_WGRAD_WANT: workgroups a weight-gradient product's split-K aims at (tuning knob)
    int scat_form = SCAT1_HALF, scat2_form = SCAT2_WAVE, sort_merge4 = 1;       // FNN_SCAT1_FORM, FNN_SCAT2_FORM, FNN_SORT_RUNS (sparse_rows.hip.h)
    int stamps = 0, stamp_sel = -1;                  // IPNN_STAMPS=1 / 2: time stamps of the wide / the tail strip launches; IPNN_STAMP_SEL=p: product p's last block
};

// main -> side: fork (start of the step), bwd (dz1 is there), wg (the weight gradients are).  side -> main: join (end of the side
// chain), tab (its table / bias half), mask (the masks).  wg and tab: IPNN_UPDATE_SIDE=1 only; mask: IPNN_MASK_SIDE=1 only.  See IpSide.
struct IpEvents { hipEvent_t fork = nullptr, bwd = nullptr, wg = nullptr, join = nullptr, tab = nullptr, mask = nullptr; };

// What a cfg alone decides of a handle's shape (ip_dims): no device, no knob but the two of ip_many_choice.
struct IpDims {
    int F = 0, K = 0, L = 0, P = 0, CB = 0, rw = SLOT; bool bf16 = false, wide = false, many_fwd = false, many_bwd = false;
    int d[IPNN_MAX_HIDDEN + 2] = {}, Dp[IPNN_MAX_HIDDEN + 2] = {};     // layer widths 0 .. L + 1, and padded
};
// The two LDS tiles of one strip launch: a strip's layers alternate between tile A and tile B, so each is as wide as the widest
// layer that lands in it over the launch's range; lds: both tiles of the launch's strip height.
struct IpTiles { int capA = 0, capB = 0; size_t lds = 0; };
constexpr size_t IP_STRIP_LDS_MAX = (size_t)160 * 1024;
// The strip side of the plan: a function of the padded widths, the element type and the knobs (ip_strip_plan), shared by
// ipnn_create and ipnn_plan_query.  Tiles of launches the handle never issues stay zero.
struct IpStrips {
    int maxD = 0;                                    // widest padded layer (sizes the pairs' exchange buffer)
    bool strip = false;                              // the strip kernels run the stack: IPNN_STRIP, and every launch below fits the LDS
    bool pairs = false;                              // ... on strips of 32 examples (bf16) with IPNN_STRIP_DUO: a batch whose pairs fit the chip takes them
    int cut = 0, maxD2 = 0;                          // products 1 .. cut are wide enough for pairs; widest layer from `cut` on
    bool splits = false;                             // a batch that runs pairs splits the stack at `cut` (IPNN_TAIL_SPLIT, 1 <= cut < L)
    IpTiles fwd, bwd;                                // the whole stack in one launch per direction
    IpTiles wide_fwd, wide_bwd;                      // products 1 .. cut as pairs of strips
    IpTiles tail_fwd, tail_bwd, tail;                // products cut + 1 .. L + 1 on 16-example strips; tail: both directions in one launch
};
// What the handle's shape and knobs decide of a step: made once, at the end of ipnn_create (ip_make_plan).  What the batch length
// adds is IpCall's (ip_form).  The cut between wide products and narrow tail: DESIGN.md section 4, round 3.
struct IpPlan : IpStrips {
    size_t off[IPNN_MAX_HIDDEN + 2] = {};            // element offset of product t's gradient in a slab (index t - 1); off[L + 1]: a slab's elements
    int wg_order[IPNN_MAX_HIDDEN + 1] = {};          // the products by size, widest first: the order of the grouped weight-gradient launch
    GemmGroupArgs group{};                           // that launch's arguments, all but nkt (the batch's k-steps)
    IpUpdArgs upd{};                                 // k_ip_update_all's, all but lr, ngb and Ba
    int mask_cols64[IPNN_MAX_HIDDEN + 1] = {};       // tiles of layer t's keep-mask per 64 examples (ip_mask_layout)
};

}  // namespace

struct ipnn_handle {
    ipnn_cfg cfg{}; std::string err; int dev = 0; hipStream_t st = nullptr; bool own_stream = false;
    int F = 0, K = 0, L = 0, P = 0, CB = 0, Bmax = 0, ldT = 0; bool bf16 = false; int splitk = 8;   // splitk: slab capacity
    IpKnobs kn; IpDims dims; IpPlan plan;             // dims: the cfg's shape (ip_dims), copied into F, K, L ... d, Dp below
    bool wide = false;                           // k >= 17: wide rows (k_ip_fwd_w / k_ip_bwd_w, k_ip_scatw1 / k_ip_scatw2), chosen at create
    int rw = SLOT;                               // row stride of the table and field stride of layer 0: SLOT, or rup(k, 4) when wide
    int* noshare = nullptr;                      // wide: [n_rows] zeros, the wide scatter's tag_shared (a row belongs to one field)
    bool many_fwd = false, many_bwd = false;     // 33 .. 64 fields of narrow rows: k_ip_fwd_m / k_ip_bwd_m (each chosen at create: ip_many_choice)
    unsigned short* ptab = nullptr;              // many: [P] pair n -> i | j << 8
    std::vector<int> sk;                         // split-K of each layer's weight-gradient product
    bool adam = false; int64_t adam_t = 0;       // Adam / FTRL: two state tensors beside every variable, dense row-gradient table; step count
    bool ftrl = false;
    bool loss_mean = false;                      // ipnn_set_loss_mean: the loss is the batch MEAN (gradients scaled by 1 / B)
    std::vector<float*> Wm, Wv; float *tm = nullptr, *tv = nullptr, *tG = nullptr, *bmv = nullptr;
    std::vector<int> d, Dp;                      // d[0..L+1], padded
    float* table16 = nullptr; int64_t n_rows = 0; float* b = nullptr;
    std::vector<float*> W; std::vector<void*> wf, wb;           // W[t], t = 1..L+1 (index t-1)
    std::vector<void*> a, aT, dl, dlT;                           // a[t] t=0..L ; dl[t] t=1..L+1 (index t-1)
    std::vector<uint8_t*> maskT;                                 // keep-masks of a step, transposed [Dp_t][ldT], t = 0..L
    uint8_t* mask0 = nullptr;                                    // drawn steps: layer 0's mask row-major [max_batch][d_0] (k_mask_draw -> IpArgs::mask); made by the first one
    // side stream (IPNN_SIDE_STREAM=0: none, everything in line): the id grouping from the start of the step; the inner-product
    // backward, the scalar b and the sparse-row update beside the weight gradients (IpSide).  With IPNN_UPDATE_SIDE=1 a step leaves
    // its dense update running there: tab_pending / upd_pending say what the main stream has not waited for yet (ip_join)
    hipStream_t st2 = nullptr; IpEvents ev;
    bool tab_pending = false, upd_pending = false;
    float* emb = nullptr;                            // [ldT][F*rw] raw embeddings of the step's examples (forward -> backward)
    float *dz0 = nullptr, *gxp = nullptr, *gb_part = nullptr, *loss_t = nullptr, *loss_dev = nullptr, *slab = nullptr;
    int* ref0 = nullptr; int* err_flag = nullptr;
    RowGroupBufs rg; void* skeys = nullptr;          // the batch's grouping (sparse_rows.hip.h); skeys: phase-A output of the split sort
    double* cpow1 = nullptr; bool key64 = true;
    size_t slab_stride = 0;
    bool prof = false;                               // HIP-event timing of the step's segments
    long long* stamps = nullptr;                     // IPNN_STAMPS: [2][Ba/16][16] time stamps of the strip kernels
    unsigned long long* duo_xch = nullptr; int* duo_flags = nullptr; int duo_epoch = 0; size_t duo_xch_wg = 0; int n_cu = 256;
    bool duo_failed = false;                         // a pair gave up once: every later train step is refused until the handle is re-created
    // ipnn_predict_multi / ipnn_eval_multi, used when this handle is hs[0]: the argument ring, the event that joins the members'
    // streams, and the scratch of one group of models (predictions, metric pass, results), kept while it is large enough
    ArgRing eval_ring{sizeof(IpGroupArg<float>), 4 * IPNN_EVAL_MAX_MODELS};
    hipEvent_t join = nullptr; char* ev_scratch = nullptr; size_t ev_scratch_bytes = 0;
    // ipnn_train_step_multi, used when this handle is hs[0]: the members' records (four calls of IPNN_STEP_MAX_MODELS members)
    // and the packed results of one call, [n_models][2] floats (loss sum, range flag), on the device and pinned on the host
    ArgRing step_ring{sizeof(IpStepArg<float>), 4 * IPNN_STEP_MAX_MODELS};
    float* step_pack = nullptr; float* step_pack_host = nullptr;
    std::map<std::string, std::vector<std::pair<hipEvent_t, hipEvent_t>>> prof_ev;
};

namespace {
struct IpProf {                                      // one segment of ip_run on the handle's stream
    ipnn_handle* h; const char* name; hipStream_t s; hipEvent_t b = nullptr, e = nullptr;
    IpProf(ipnn_handle* h_, const char* n, hipStream_t s_ = nullptr) : h(h_), name(n), s(s_ ? s_ : h_->st) {
        if (!h->prof) return;
        hipEventCreate(&b); hipEventCreate(&e); hipEventRecord(b, s);
    }
    ~IpProf() { if (!h->prof) return; hipEventRecord(e, s); h->prof_ev[name].emplace_back(b, e); }
};
}

#define IHK(h, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_); return FNN_ERR_HIP; } } while (0)
#define IFAIL(h, code, msg) do { (h)->err = (msg); return (code); } while (0)
#define IRC(expr) do { const int rc_ = (expr); if (rc_ != FNN_OK) return rc_; } while (0)

namespace {

size_t ts(const ipnn_handle* h) { return h->bf16 ? 2 : 4; }

template <typename T> void ip_refresh(ipnn_handle* h, int t, const float* slab, float lr) {      // t = 1..L+1
    const int Din = h->Dp[t - 1], Dout = h->Dp[t];
    const size_t n = (size_t)Din * Dout;
    hipLaunchKernelGGL((k_ip_update<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->W[t - 1], slab, h->sk[t - 1],
                       h->slab_stride, lr, Din, Dout, (T*)h->wf[t - 1], (T*)h->wb[t - 1]);
}

inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

IpKnobs ip_read_knobs()
{
    IpKnobs k;
    const struct { const char* name; int* v; bool flag; } plain[] = {     // flag: 0 / 1, whatever number is given
        {"IPNN_SIDE_STREAM", &k.side_stream, true}, {"IPNN_UPDATE_SIDE", &k.upd_side, true}, {"IPNN_MASK_SIDE", &k.mask_side, false},
        {"IPNN_STRIP", &k.strip, true}, {"IPNN_STRIP_L0", &k.strip_l0, true}, {"IPNN_GEMM_LDS", &k.gemm_lds, true}, {"IPNN_STRIP_DUO", &k.duo, false}, {"IPNN_DUO_MIN", &k.duo_min, false},
        {"IPNN_TAIL_SPLIT", &k.tail_split, false}, {"IPNN_TAIL_FUSE", &k.tail_fuse, true}, {"IPNN_TAIL_LDS", &k.tail_w_lds, false},
        {"IPNN_STRIP_ROT", &k.strip_rot, false}, {"IPNN_FWD_SKIP", &k.fwd_skip, false}, {"IPNN_STRIP_WARM", &k.strip_warm, false},
        {"IPNN_GROUP_WGRAD", &k.group_wgrad, true}, {"IPNN_GROUP_XCD", &k.group_xcd, false}, {"IPNN_STAMP_SEL", &k.stamp_sel, false}};
    for (const auto& e : plain) { *e.v = env_int(e.name, *e.v); if (e.flag) *e.v = *e.v != 0; }
    k.wt = env_int("IPNN_WT", 1) != 0;
    k.duo_min = std::max(2, k.duo_min);
    { const int v = env_int("IPNN_TAIL_NF", 1); if (v == 1 || v == 2 || v == 4) k.tail_nf = v; }
    k.tail_nw = env_int("IPNN_TAIL_NW", 16) == 16 ? 16 : 8;
    k.ipf_nt = env_int("IPNN_IPF_NT", 1024) == 1024 ? 1024 : 512;
    int nf = 4, nw = 8;
    if (getenv("IPNN_WIDE") && sscanf(getenv("IPNN_WIDE"), "%d:%d", &nf, &nw) == 2 && ((nf == 2 && (nw == 8 || nw == 12)) || (nf == 4 && nw == 8))) { k.wide_nf = nf; k.wide_nw = nw; }
    // one launch per product wants ~256 workgroups each; the grouped launch runs all products side by side and is
    // served best by half of that (measured: 0.353 -> 0.345 ms/step; a quarter: 0.355)
    k.wgrad_want = getenv("IPNN_WGRAD_WANT") ? std::max(16, env_int("IPNN_WGRAD_WANT", 0)) : k.group_wgrad ? 144 : 288;
    k.scat_form = scat1_form_env(); k.scat2_form = scat2_form_env(); k.sort_merge4 = sort_merge4_env(1);
    if (getenv("IPNN_STAMPS")) k.stamps = env_int("IPNN_STAMPS", 0) == 2 ? 2 : 1;
    return k;
}

// The main stream waits for what the previous step left running on the side stream (IPNN_UPDATE_SIDE=1): its sparse rows and bias
// (read by the gather) ...
int ip_join_table(ipnn_handle* h)
{
    if (h->tab_pending) { IHK(h, hipStreamWaitEvent(h->st, h->ev.tab, 0)); h->tab_pending = false; }
    return FNN_OK;
}
// ... and its dense update (read by the first product, and by every other entry point)
int ip_join(ipnn_handle* h)
{
    IRC(ip_join_table(h));
    if (h->upd_pending) { IHK(h, hipStreamWaitEvent(h->st, h->ev.join, 0)); h->upd_pending = false; }
    return FNN_OK;
}

// The side stream of one step, as a scope.  fork: the side stream waits for what the main stream holds so far; signal: an event
// at the side stream's end; wait: the main stream waits for it.  Without a side stream (IPNN_SIDE_STREAM=0) `s` is the main stream
// and all three do nothing.  A step that ends well calls settle(): its last wait is enqueued, or tab_pending / upd_pending hand it
// to the next call.  Any other exit after the first fork -- every error return of ip_run -- joins here: the main stream waits for
// whatever the step put on the side stream, so that no later call on the handle's stream races with it.
struct IpSide {
    ipnn_handle* const h; hipStream_t const s; bool open = false;
    explicit IpSide(ipnn_handle* h_) : h(h_), s(h_->st2 ? h_->st2 : h_->st) {}
    IpSide(const IpSide&) = delete;
    bool on() const { return h->st2 != nullptr; }
    int fork(hipEvent_t ev)
    {
        if (!on()) return FNN_OK;
        IHK(h, hipEventRecord(ev, h->st));
        open = true;
        IHK(h, hipStreamWaitEvent(h->st2, ev, 0));
        return FNN_OK;
    }
    int signal(hipEvent_t ev) { if (on()) IHK(h, hipEventRecord(ev, h->st2)); return FNN_OK; }
    int wait(hipEvent_t ev) { if (on()) IHK(h, hipStreamWaitEvent(h->st, ev, 0)); return FNN_OK; }
    void settle() { open = false; }
    ~IpSide() { if (open && hipEventRecord(h->ev.join, h->st2) == hipSuccess) hipStreamWaitEvent(h->st, h->ev.join, 0); }
};

// ---------------------------------------------------------------------------------------------------------------- kernel selectors
// A launchable kernel: what a selector returns.  The selectors below are the only places that name an instantiation of the strip
// and gather kernels; the launch sites call them, and so does the dynamic-LDS opt-in (ip_opt_in), over every form the knobs can
// select: what can be launched has its attribute.
struct IpKernel { const void* fn; int threads; };
#define IP_K(threads, ...) IpKernel{reinterpret_cast<const void*>(&__VA_ARGS__), (threads)}

// args: the kernel's parameters, in order and of exactly its parameter types
template <typename... A> hipError_t ip_launch(const IpKernel& k, dim3 grid, size_t lds, hipStream_t s, const A&... args)
{
    void* p[] = {const_cast<void*>(static_cast<const void*>(&args))...};
    return hipLaunchKernel(k.fn, grid, dim3((unsigned)k.threads), p, lds, s);
}

// The strip kernels of one direction by (rt: rows of 16 examples per strip, nf: 16-column fragments per item, nw: waves).  Built:
// 32-example strips (bf16) as 4:8 -- the whole stack in one launch, and IPNN_WIDE=4:8 --, 2:8 and 2:12 (half-block items; measured:
// forward 59.8 -> 56.4 us at 2:8); 16-example strips (every f32 launch, every tail) as 4:8, 2:8, 1:8 and 1:16.  What is not built
// takes nf:nw = 4:8, and f32 has no 32-example strips (it ignores IPNN_WIDE).
template <typename T> IpKernel ip_strip_sel(bool bwd, int rt, int nf, int nw)
{
#define IP_STRIP(RT_, NF, NW) (bwd ? IP_K(64 * NW, k_ip_strip_bwd<T, RT_, NF, NW>) : IP_K(64 * NW, k_ip_strip_fwd<T, RT_, NF, NW>))
    if constexpr (sizeof(T) == 2) if (rt == 2) {
        if (nf == 2 && nw == 12) return IP_STRIP(2, 2, 12);
        if (nf == 2 && nw == 8) return IP_STRIP(2, 2, 8);
        return IP_STRIP(2, 4, STRIP_NW);
    }
    if (nf == 1 && nw == 16) return IP_STRIP(1, 1, 16);
    if (nf == 1) return IP_STRIP(1, 1, STRIP_NW);
    if (nf == 2) return IP_STRIP(1, 2, STRIP_NW);
    return IP_STRIP(1, 4, STRIP_NW);
#undef IP_STRIP
}
// both passes' tails in one launch: the fused form's only instantiation (1 fragment per item on 16 waves)
template <typename T> IpKernel ip_strip_tail_sel() { return IP_K(64 * 16, k_ip_strip_tail<T, 1, 16>); }

// Which inner-product (gather) kernels a handle runs, per direction: wide rows (k >= 17), many fields (ip_many_choice), or the
// 16-example pair k_ip_fwd / k_ip_bwd
enum IpRows { IP_NARROW, IP_WIDE, IP_MANY };
IpRows ip_fwd_rows(const ipnn_handle* h) { return h->wide ? IP_WIDE : h->many_fwd ? IP_MANY : IP_NARROW; }
IpRows ip_bwd_rows(const ipnn_handle* h) { return h->wide ? IP_WIDE : h->many_bwd ? IP_MANY : IP_NARROW; }
// examples per workgroup of the handle's inner-product backward: the grain of gb_part
int ip_bwd_ex(const ipnn_handle* h) { return h->wide ? IPW_EX : h->many_bwd ? IPM_BEX : 16; }
// ceiling of their dynamic LDS: one per kernel family, for every handle (the attribute belongs to the kernel, not to the handle; the
// widest wide shape takes 132 / 147 KB, the 16-example tile up to 160 KiB: ip_many_choice)
int ip_rows_lds_kib(IpRows r) { return r == IP_MANY ? 64 : 160; }

// wv: value weights are given.  A compile-time variant, so that the unweighted path carries neither the loads nor a branch.
template <typename T> IpKernel ip_gather_fwd_sel(IpRows rows, bool wv, int nt)
{
    if (rows == IP_WIDE) return wv ? IP_K(256, k_ip_fwd_w<T, true>) : IP_K(256, k_ip_fwd_w<T>);
    if (rows == IP_MANY) return wv ? IP_K(256, k_ip_fwd_m<T, true>) : IP_K(256, k_ip_fwd_m<T>);
    if (nt == 1024) return wv ? IP_K(1024, k_ip_fwd<T, 1024, true>) : IP_K(1024, k_ip_fwd<T, 1024>);
    return wv ? IP_K(IPF_NT, k_ip_fwd<T, IPF_NT, true>) : IP_K(IPF_NT, k_ip_fwd<T>);
}
// the group forms (ipnn_predict_multi / ipnn_eval_multi): the gather of a row kind, and the whole stack on single strips
template <typename T> IpKernel ip_gather_fwd_g_sel(IpRows rows, bool wv, int nt)
{
    if (rows == IP_WIDE) return wv ? IP_K(256, k_ip_fwd_w_g<T, true>) : IP_K(256, k_ip_fwd_w_g<T, false>);
    if (rows == IP_MANY) return wv ? IP_K(256, k_ip_fwd_m_g<T, true>) : IP_K(256, k_ip_fwd_m_g<T, false>);
    if (nt == 1024) return wv ? IP_K(1024, k_ip_fwd_g<T, 1024, true>) : IP_K(1024, k_ip_fwd_g<T, 1024, false>);
    return wv ? IP_K(IPF_NT, k_ip_fwd_g<T, IPF_NT, true>) : IP_K(IPF_NT, k_ip_fwd_g<T, IPF_NT, false>);
}
template <typename T> IpKernel ip_strip_g_sel() { return IP_K(64 * STRIP_NW, k_ip_strip_fwd_g<T, sizeof(T) == 2 ? 2 : 1>); }
// the group forms of the training step (ipnn_train_step_multi; narrow rows, by row kind per direction): the gather that also
// writes the T layout and the embeddings, the whole stack on single strips in either direction, the inner products' backward
template <typename T> IpKernel ip_step_gather_sel(IpRows rows, bool wv, int nt)
{
    if (rows == IP_MANY) return wv ? IP_K(256, k_ip_fwd_m_tg<T, true>) : IP_K(256, k_ip_fwd_m_tg<T, false>);
    if (nt == 1024) return wv ? IP_K(1024, k_ip_fwd_tg<T, 1024, true>) : IP_K(1024, k_ip_fwd_tg<T, 1024, false>);
    return wv ? IP_K(IPF_NT, k_ip_fwd_tg<T, IPF_NT, true>) : IP_K(IPF_NT, k_ip_fwd_tg<T, IPF_NT, false>);
}
template <typename T> IpKernel ip_step_strip_sel(bool bwd)
{
    constexpr int RT = sizeof(T) == 2 ? 2 : 1;
    return bwd ? IP_K(64 * STRIP_NW, k_ip_strip_bwd_g<T, RT>) : IP_K(64 * STRIP_NW, k_ip_strip_fwd_tg<T, RT>);
}
template <typename T> IpKernel ip_step_bwd_sel(IpRows rows, bool wv)
{
    if (rows == IP_MANY) return wv ? IP_K(256, k_ip_bwd_m_g<T, true>) : IP_K(256, k_ip_bwd_m_g<T, false>);
    return wv ? IP_K(256, k_ip_bwd_g<T, true>) : IP_K(256, k_ip_bwd_g<T, false>);
}
IpKernel ip_gather_bwd_sel(IpRows rows, bool wv)
{
    if (rows == IP_WIDE) return wv ? IP_K(256, k_ip_bwd_w<true>) : IP_K(256, k_ip_bwd_w<false>);
    if (rows == IP_MANY) return wv ? IP_K(256, k_ip_bwd_m<true>) : IP_K(256, k_ip_bwd_m<false>);
    return wv ? IP_K(256, k_ip_bwd<true>) : IP_K(256, k_ip_bwd<false>);
}

// > 64 KiB of dynamic LDS needs the opt-in, once per device: every kernel a selector can return for a form the knobs can name gets
// its family's ceiling -- 160 KiB for the strips and the fused tail (IP_STRIP_LDS_MAX: what ip_strip_plan holds every launch to),
// ip_rows_lds_kib for the gathers.  (A form named twice is set twice: the same value.)
template <typename T> int ip_opt_in(ipnn_handle* h)
{
    constexpr int RT = sizeof(T) == 2 ? 2 : 1;
    auto set = [](const IpKernel& k, int kib) { return hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, kib * 1024); };
    for (int bwd = 0; bwd < 2; ++bwd)
        for (int rt : {RT, 1}) for (int nf : {1, 2, 4}) for (int nw : {8, 12, 16})
            IHK(h, set(ip_strip_sel<T>(bwd != 0, rt, nf, nw), 160));
    IHK(h, set(ip_strip_tail_sel<T>(), 160));
    for (IpRows r : {IP_NARROW, IP_WIDE, IP_MANY}) for (int wv = 0; wv < 2; ++wv) {
        for (int nt : {512, 1024}) IHK(h, set(ip_gather_fwd_sel<T>(r, wv != 0, nt), ip_rows_lds_kib(r)));
        for (int nt : {512, 1024}) IHK(h, set(ip_gather_fwd_g_sel<T>(r, wv != 0, nt), ip_rows_lds_kib(r)));
        IHK(h, set(ip_gather_bwd_sel(r, wv != 0), ip_rows_lds_kib(r)));
    }
    IHK(h, set(ip_strip_g_sel<T>(), 160));
    for (IpRows r : {IP_NARROW, IP_MANY}) for (int wv = 0; wv < 2; ++wv) {
        for (int nt : {512, 1024}) IHK(h, set(ip_step_gather_sel<T>(r, wv != 0, nt), ip_rows_lds_kib(r)));
        IHK(h, set(ip_step_bwd_sel<T>(r, wv != 0), ip_rows_lds_kib(r)));
    }
    for (int bwd = 0; bwd < 2; ++bwd) IHK(h, set(ip_step_strip_sel<T>(bwd != 0), 160));
    return FNN_OK;
}

// ------------------------------------------------------------------------------------------------------------------ the step plan
// Which inner-product kernels a narrow handle runs.  Up to 32 fields: always the 16-example pair (k_ip_fwd / k_ip_bwd).  Above,
// each direction has its own crossover, both measured: the 4-example backward wins from 33 fields on
// (IPM_BWD_MIN_FIELDS; IPNN_MANY_MIN is the A/B knob), the 16-example forward wins wherever its tile fits the 160 KiB of LDS,
// so the 8-example forward takes over where it does not: 46 fields and more with pairs (IPM_FWD_MIN_FIELDS = 65 means "by LDS
// only"; IPNN_MANY_FWD_MIN is the A/B knob).  Neither knob goes below 33.
constexpr int IPM_BWD_MIN_FIELDS = 33, IPM_FWD_MIN_FIELDS = 65;
inline size_t ip16_lds(int F, int Dp0) { return (size_t)16 * (F * (SLOT + 1) + Dp0) * sizeof(float); }      // k_ip_fwd pads its embedding tile
inline bool ip_many_choice(int F, int Dp0, int dflt, const char* knob)
{
    if (F <= 32) return false;
    const int mn = getenv(knob) ? std::max(33, env_int(knob, 0)) : dflt;
    return F >= mn || ip16_lds(F, Dp0) > (size_t)160 * 1024;
}

// What ipnn_create refuses of a cfg for its shape (the message: g_ip_err).  No device is asked.
int ip_cfg_check(const ipnn_cfg* cfg)
{
    if (cfg->k < 1 || cfg->k > 128) {
        g_ip_err = "bad shape: k = " + std::to_string(cfg->k) + " (k = rank+1 must be 1..128)"; return FNN_ERR_ARG; }
    if (cfg->n_fields < 2 || cfg->n_fields > 64) {
        g_ip_err = "bad shape: n_fields = " + std::to_string(cfg->n_fields) + " (2..64 fields of k <= 16, 2..32 fields of k = 17..128: more is not built)"; return FNN_ERR_ARG; }
    if (cfg->k > SLOT && cfg->n_fields > 32) {
        g_ip_err = "bad shape: n_fields = " + std::to_string(cfg->n_fields) + " with k = " + std::to_string(cfg->k) +
                   " (wide rows, k = 17..128, take 2..32 fields: more than 32 is not built; k <= 16 takes 2..64)"; return FNN_ERR_ARG; }
    if (cfg->n_hidden < 1 || cfg->n_hidden > IPNN_MAX_HIDDEN ||
        cfg->max_batch < 1 || cfg->max_batch > 4096 || !(cfg->keep_prob > 0.f && cfg->keep_prob <= 1.f)) {
        g_ip_err = "bad shape (2..64 fields of k <= 16 or 2..32 fields of k = 17..128, 1..8 hidden layers, batch <= 4096, 0 < keep_prob <= 1)"; return FNN_ERR_ARG; }
    if (cfg->act != A_TANH && cfg->act != A_SIG && cfg->act != A_RELU) { g_ip_err = "bad act"; return FNN_ERR_ARG; }
    if (cfg->precision != FNN_PREC_F32 && cfg->precision != FNN_PREC_BF16) { g_ip_err = "bad precision (FNN_PREC_F32 or FNN_PREC_BF16; FNN_PREC_BF16X3 is the FNN / SNN engine's)"; return FNN_ERR_ARG; }
    if (cfg->optimizer != IPNN_OPT_SGD && cfg->optimizer != IPNN_OPT_ADAM && cfg->optimizer != IPNN_OPT_FTRL) { g_ip_err = "bad optimizer"; return FNN_ERR_ARG; }
    if (cfg->optimizer == IPNN_OPT_ADAM && !(cfg->adam_eps > 0.f)) { g_ip_err = "Adam needs adam_eps > 0"; return FNN_ERR_ARG; }
    for (int t = 0; t < cfg->n_hidden; ++t) if (cfg->hidden[t] < 1 || cfg->hidden[t] > 4095) { g_ip_err = "hidden size out of range"; return FNN_ERR_ARG; }
    return FNN_OK;
}

// the shape of a checked cfg: row layout, layer widths and their padding, the inner-product kernels per direction
IpDims ip_dims(const ipnn_cfg& cfg)
{
    IpDims m;
    m.F = cfg.n_fields; m.K = cfg.k; m.L = cfg.n_hidden; m.bf16 = cfg.precision == FNN_PREC_BF16;
    m.wide = m.K > SLOT; m.rw = m.wide ? rup(m.K, 4) : SLOT;
    m.P = cfg.pairs ? m.F * (m.F - 1) / 2 : 0; m.CB = m.F * m.rw + m.P;
    m.d[0] = m.F * m.K + m.P + 1; m.Dp[0] = rup(m.CB + 2, 64);
    for (int t = 1; t <= m.L; ++t) { m.d[t] = cfg.hidden[t - 1]; m.Dp[t] = rup(m.d[t] + 1, 64); }
    m.d[m.L + 1] = 1; m.Dp[m.L + 1] = 64;
    m.many_fwd = !m.wide && ip_many_choice(m.F, m.Dp[0], IPM_FWD_MIN_FIELDS, "IPNN_MANY_FWD_MIN");
    m.many_bwd = !m.wide && ip_many_choice(m.F, m.Dp[0], IPM_BWD_MIN_FIELDS, "IPNN_MANY_MIN");
    return m;
}

// The tiles of a launch that keeps m + 1 layers in LDS, the i-th of them Dp[first + i * dir] columns wide: even i in tile A, odd
// i in tile B.  rows_bytes: a column of a strip (16 or 32 examples of the element type).
IpTiles ip_tiles_of(const int* Dp, int first, int dir, int m, size_t rows_bytes)
{
    IpTiles t;
    for (int i = 0; i <= m; ++i) { int& cap = (i & 1) ? t.capB : t.capA; cap = std::max(cap, Dp[first + i * dir]); }
    t.lds = rows_bytes * (size_t)(t.capA + t.capB);
    return t;
}
// Forward over Dp[lo .. lo + n]: the strip of layer lo in tile A, then one layer per product; the output unit (has_out) is never tiled.
IpTiles ip_tiles_fwd(const int* Dp, int lo, int n, bool has_out, size_t rows_bytes) { return ip_tiles_of(Dp, lo, 1, has_out ? n - 1 : n, rows_bytes); }
// Backward over Dp[lo .. lo + n]: delta l_{lo + n} in tile A, then downwards; the stack's bottom (dz1: f32, row-major, to memory) is never tiled.
IpTiles ip_tiles_bwd(const int* Dp, int lo, int n, bool bottom, size_t rows_bytes) { return ip_tiles_of(Dp, lo + n, -1, bottom ? n - 1 : n, rows_bytes); }

// Which launches run the deep stack, and their tiles.  Up to 32 fields, and up to a layer 0 of 1024 columns: two equal tiles as
// wide as the widest layer of the launch's range, and strips while they fit 128 KiB.  A wider layer 0 of more than 32 fields
// (33 and more with pairs, 64 without): each launch gets the two widths its own layers need -- layer 0 is in a tile only going forward, and then it
// never shares one with layer 1 -- and the handle runs strips when every launch of its forms fits the 160 KiB of LDS.
// IPNN_STRIP_L0=0 keeps the first rule for every handle.
IpStrips ip_strip_plan(const IpDims& m, const IpKnobs& kn)
{
    IpStrips p;
    const int L = m.L, *Dp = m.Dp;
    const int RT = m.bf16 ? 2 : 1;                               // strip = 32 (bf16) / 16 (f32) examples
    const size_t es = m.bf16 ? 2 : 4, rows = (size_t)RT * 16 * es, rows16 = 16 * es;
    for (int t = 0; t <= L + 1; ++t) p.maxD = std::max(p.maxD, Dp[t]);
    p.cut = L;
    while (p.cut >= 1 && Dp[p.cut] / 64 < kn.duo_min) --p.cut;
    for (int t = p.cut; t <= L + 1; ++t) p.maxD2 = std::max(p.maxD2, Dp[t]);
    const bool pairs = kn.duo && RT == 2, splits = pairs && kn.tail_split && p.cut >= 1 && p.cut < L;
    const bool equal_tiles = m.F <= 32 || Dp[0] <= 1024 || !kn.strip_l0;
    auto equal = [](int w, size_t rb) { return IpTiles{w, w, 2 * rb * (size_t)w}; };
    IpStrips q = p;
    if (equal_tiles) {
        q.fwd = q.bwd = equal(p.maxD, rows);
        if (splits) { q.wide_fwd = q.wide_bwd = q.fwd; q.tail_fwd = q.tail_bwd = q.tail = equal(p.maxD2, rows16); }
        q.strip = kn.strip && q.fwd.lds <= (size_t)128 * 1024;
    } else {
        q.fwd = ip_tiles_fwd(Dp, 0, L + 1, true, rows); q.bwd = ip_tiles_bwd(Dp, 0, L + 1, true, rows);
        if (splits) {
            q.wide_fwd = ip_tiles_fwd(Dp, 0, p.cut, false, rows); q.wide_bwd = ip_tiles_bwd(Dp, 0, p.cut, true, rows);
            q.tail_fwd = ip_tiles_fwd(Dp, p.cut, L + 1 - p.cut, true, rows16); q.tail_bwd = ip_tiles_bwd(Dp, p.cut, L + 1 - p.cut, false, rows16);
            q.tail.capA = std::max(q.tail_fwd.capA, q.tail_bwd.capA); q.tail.capB = std::max(q.tail_fwd.capB, q.tail_bwd.capB);
            q.tail.lds = rows16 * (size_t)(q.tail.capA + q.tail.capB);
        }
        q.strip = kn.strip;
        for (const IpTiles* t : {&q.fwd, &q.bwd, &q.wide_fwd, &q.wide_bwd, &q.tail_fwd, &q.tail_bwd, &q.tail}) q.strip = q.strip && t->lds <= IP_STRIP_LDS_MAX;
    }
    if (!q.strip) return p;                                      // the GEMM path: no strip launch, no tiles
    q.pairs = pairs; q.splits = splits;
    return q;
}
// a handle shares the launches of ipnn_train_step_multi when every stage of its solo step has a group form that computes the same
// bits: the strip kernels on narrow rows (k <= 16, any field count), the grouped weight-gradient launch, no diagnostic knob
bool ip_shares_step(const IpStrips& p, const IpDims& m, const IpKnobs& kn)
{
    return p.strip && !m.wide && kn.group_wgrad && m.L + 1 <= GEMM_GROUP_MAX && !kn.fwd_skip && !kn.stamps;
}

template <typename T> void ip_make_plan(ipnn_handle* h)
{
    IpPlan& p = h->plan;
    const IpKnobs& kn = h->kn;
    const int L = h->L;
    constexpr int KS = Traits<T>::KS;
    static_cast<IpStrips&>(p) = ip_strip_plan(h->dims, kn);
    for (int t = 0; t <= L; ++t) p.mask_cols64[t] = h->Dp[t] / 64;
    for (int t = 1; t <= L + 1; ++t) { p.off[t] = p.off[t - 1] + (size_t)h->Dp[t - 1] * h->Dp[t]; p.wg_order[t - 1] = t; }
    std::sort(p.wg_order, p.wg_order + L + 1, [&](int x, int y) { return (size_t)h->Dp[x - 1] * h->Dp[x] > (size_t)h->Dp[y - 1] * h->Dp[y]; });
    if (L + 1 <= GEMM_GROUP_MAX) {   // ONE launch for the whole stack: 128 x 128 tiles of every product, widest first
        GemmGroupArgs& g = p.group;
        int wg = 0;
        for (int i = 0; i <= L; ++i) {
            const int t = p.wg_order[i], M = h->Dp[t - 1], N = h->Dp[t];
            GemmGroupProb& pr = g.p[i];
            pr.A = h->aT[t - 1]; pr.B = h->dlT[t - 1]; pr.out = h->slab + p.off[t - 1]; pr.mt16 = M / 16; pr.nt16 = N / 16;
            pr.nkt_all = h->ldT / KS; pr.nkt = 0; pr.ldo = N; pr.gx = (M + 127) / 128; pr.gy = (N + 127) / 128;
            g.wg0[i] = wg; wg += pr.gx * pr.gy * h->sk[t - 1];
        }
        g.wg0[L + 1] = wg; g.n = L + 1; g.zstride = h->slab_stride; g.xcd = kn.group_xcd; g.wt = kn.wt;
    }
    IpUpdArgs& u = p.upd;
    u.wt = kn.wt;
    for (int t = 1; t <= L + 1; ++t) {
        u.W[t - 1] = h->W[t - 1]; u.wf[t - 1] = h->wf[t - 1]; u.wb[t - 1] = h->wb[t - 1]; u.off[t - 1] = p.off[t - 1];
        u.Din[t - 1] = h->Dp[t - 1]; u.Dout[t - 1] = h->Dp[t]; u.sk[t - 1] = h->sk[t - 1];
    }
    u.n = L + 1; u.off[L + 1] = p.off[L + 1]; u.slab = h->slab; u.zstride = h->slab_stride;
    u.adam = h->adam ? (int)h->cfg.optimizer : 0; u.beta1 = h->cfg.adam_beta1; u.beta2 = h->cfg.adam_beta2; u.eps = h->cfg.adam_eps; u.bmv = h->bmv;
    if (h->adam) for (int t = 0; t <= L; ++t) { u.Wm[t] = h->Wm[t]; u.Wv[t] = h->Wv[t]; }
    u.b = h->b; u.gb_part = h->gb_part; u.loss_t = h->loss_t; u.loss_sum = h->loss_dev; u.err = h->err_flag;
}

// Adam / FTRL start over: zero moments beside every dense layer and b, FTRL's accumulators at 0.1 (initial_accumulator_value), step
// count 0.  (The table's state is ipnn_set_table's: it is sized by the table.)
int ip_reset_dense_state(ipnn_handle* h)
{
    if (!h->adam) return FNN_OK;
    for (int t = 1; t <= h->L + 1; ++t) {
        const size_t n = (size_t)h->Dp[t - 1] * h->Dp[t];
        IHK(h, hipMemsetAsync(h->Wm[t - 1], 0, n * 4, h->st)); IHK(h, hipMemsetAsync(h->Wv[t - 1], 0, n * 4, h->st));
        if (h->ftrl) hipLaunchKernelGGL(k_fill_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->Wm[t - 1], n, 0.1f);
    }
    IHK(h, hipMemsetAsync(h->bmv, 0, 8, h->st));
    if (h->ftrl) hipLaunchKernelGGL(k_fill_f32, dim3(1), dim3(64), 0, h->st, h->bmv, (size_t)1, 0.1f);
    h->adam_t = 0;
    return FNN_OK;
}

// ------------------------------------------------------------------------------------------------------------------- one call
// masks: the caller's keep-masks (ipnn_train_step_w), or draw: the (seed, step) the library draws them from (ipnn_train_step_drawn);
// neither: no dropout.  wts: value weights [B][F] (device) or NULL: the kernels as they were before the weights existed.
struct IpDraw { uint64_t seed, step; };
struct IpCall {
    const int32_t* ids; const float* wts; const float* y; int B; const uint8_t* const* masks; const IpDraw* draw;
    float* logits_out; float* p_out; bool train;
    // what the batch length makes of the plan (ip_form)
    int Ba = 0, nstrips = 0; bool duo = false, tsplit = false, fuse_tail = false;
    bool drop = false; const uint8_t* mask0 = nullptr;      // dropout at all; layer 0's mask, row-major (the inner-product forward)
};

void ip_form(const ipnn_handle* h, IpCall& c)
{
    const IpPlan& p = h->plan;
    const IpKnobs& kn = h->kn;
    c.Ba = rup(c.B, 256);
    c.nstrips = c.Ba / (16 * (h->bf16 ? 2 : 1));
    // two workgroups per strip (StripDuo) where the pairs fit the chip at one workgroup per CU: both halves of a pair must be
    // resident to swap (bf16 strips of 32 examples: 256 workgroups at batch 4096)
    c.duo = p.pairs && 2 * c.nstrips <= h->n_cu;
    c.tsplit = c.duo && p.splits;
    // training steps: the forward tail rides in the backward tail's launch (k_ip_strip_tail; IPNN_TAIL_FUSE=0: two launches)
    c.fuse_tail = c.tsplit && c.train && kn.tail_fuse && kn.tail_nf == 1 && kn.tail_nw == 16 && !kn.tail_w_lds;
    c.drop = c.train && (c.masks || c.draw);
    c.mask0 = !c.drop ? nullptr : c.draw ? h->mask0 : c.masks[0];
}

// The tiles of every layer's keep-mask, 64 examples x 64 columns each, layer after layer: the grid of k_mask_T and k_mask_draw and
// the fields their argument structs share.  Returns the number of tiles.
template <typename A> int ip_mask_layout(const ipnn_handle* h, int B, A& a)
{
    const int Ba = rup(B, 256);
    int tiles = 0;
    for (int t = 0; t <= h->L; ++t) { a.d[t] = h->d[t]; a.Dp[t] = h->Dp[t]; a.tile0[t] = tiles; tiles += (Ba / 64) * h->plan.mask_cols64[t]; }
    a.tile0[h->L + 1] = tiles; a.n = h->L + 1; a.ref0 = h->ref0; a.B = B; a.Ba = Ba; a.ldT = h->ldT; a.wt = h->kn.wt;
    return tiles;
}
// the launch arguments of k_mask_draw for one (seed, step): the layout, the key, the counter's step words and the threshold of the
// handle's keep_prob; the targets (dstT / dstR) are the caller's to fill in
MaskDrawArgs ip_draw_args(const ipnn_handle* h, const IpDraw& dr, int B, int* tiles_out)
{
    MaskDrawArgs a{};
    *tiles_out = ip_mask_layout(h, B, a);
    for (int t = 0; t <= h->L; ++t) a.bytesT[t] = (unsigned)((size_t)h->ldT * h->Dp[t]);
    a.key0 = (unsigned)dr.seed; a.key1 = (unsigned)(dr.seed >> 32); a.step0 = (unsigned)dr.step; a.step1 = (unsigned)(dr.step >> 32);
    const double thr = std::floor((double)h->cfg.keep_prob * 4294967296.0);
    a.all = h->cfg.keep_prob >= 1.0f;
    a.thr = thr >= 4294967295.0 ? 0xffffffffu : (unsigned)thr;
    return a;
}

// The step's keep-masks where the launches read them: the library's own draw (transposed, and layer 0's row-major, written by one
// launch that reads nothing), or the caller's, transposed, tiled, zero padded and slot-ordered for layer 0.
// On the MAIN stream by default: a cross-stream event on the way into the first strip kernel costs more (10-20 us of wait
// resolution, measured on the kernel trace) than the 10 us the transposition takes in line (IPNN_MASK_SIDE=1; DESIGN.md section 4
// also tells of transposing the NEXT step's masks ahead: not kept).
// a training step's draw: every layer's transposed mask, and layer 0's row-major as well
MaskDrawArgs ip_step_draw_args(const ipnn_handle* h, const IpCall& c, int* tiles_out)
{
    MaskDrawArgs da = ip_draw_args(h, *c.draw, c.B, tiles_out);
    for (int t = 0; t <= h->L; ++t) da.dstT[t] = h->maskT[t];
    da.dstR[0] = h->mask0;
    return da;
}
// ... and the transposition of the caller's masks
MaskTArgs ip_step_maskT_args(const ipnn_handle* h, const IpCall& c, int* tiles_out)
{
    MaskTArgs ma{};
    *tiles_out = ip_mask_layout(h, c.B, ma);
    for (int t = 0; t <= h->L; ++t) { ma.src[t] = c.masks[t]; ma.dst[t] = h->maskT[t]; }
    return ma;
}
int ip_masks(ipnn_handle* h, const IpCall& c, IpSide& side)
{
    if (!c.drop) return FNN_OK;
    hipStream_t ms = h->kn.mask_side ? side.s : h->st;
    IpProf pm(h, "mask_t", ms);
    int tiles = 0;
    if (c.draw) {
        const MaskDrawArgs da = ip_step_draw_args(h, c, &tiles);
        hipLaunchKernelGGL(k_mask_draw, dim3(tiles), dim3(256), 0, ms, da);
    } else {
        const MaskTArgs ma = ip_step_maskT_args(h, c, &tiles);
        hipLaunchKernelGGL(k_mask_T, dim3(tiles), dim3(256), 0, ms, ma);
    }
    if (h->kn.mask_side) IRC(side.signal(h->ev.mask));
    return FNN_OK;
}

// the grouping of the batch's ids for the sparse-row update (needed by the scatter): beside the stack, on the side stream
void ip_sort_ids(ipnn_handle* h, const IpCall& c, hipStream_t ss)
{
    SortArgs so{c.ids, c.B, h->F, h->n_rows, h->rg.rec, h->rg.owner_cnt, h->F, h->skeys};
    so.merge4 = h->kn.sort_merge4;
    launch_sort(ss, h->key64, so);
}

// the 16-example gather's arguments (narrow rows, up to 32 fields)
IpFwdArgs ip_fwd_args(const ipnn_handle* h, const IpCall& c, const uint8_t* mask0, float inv_keep)
{
    return IpFwdArgs{h->P, c.ids, c.B, h->F, h->K, h->table16, h->n_rows, h->b, mask0, h->d[0],
                     inv_keep, h->cfg.act, h->Dp[0], h->ldT, h->err_flag, h->kn.fwd_skip, h->kn.wt, c.wts};
}

IpManyArgs ip_many_args(const ipnn_handle* h, const IpCall& c, const uint8_t* mask0, float inv_keep)
{
    return IpManyArgs{h->P, c.ids, c.B, h->F, h->K, h->table16, h->n_rows, h->b, mask0, h->d[0], inv_keep, h->cfg.act, h->Dp[0], h->ldT,
                      h->err_flag, h->ptab, h->kn.wt, (unsigned)((size_t)h->ldT * h->Dp[0] * ts(h)), (unsigned)((size_t)h->ldT * h->F * SLOT * 4), c.wts};
}
IpWideArgs ip_wide_args(const ipnn_handle* h, const IpCall& c, const uint8_t* mask0, float inv_keep)
{
    return IpWideArgs{h->P, c.ids, c.B, h->F, h->K, h->rw, h->table16, h->n_rows, h->b, mask0, h->d[0], inv_keep, h->cfg.act, h->Dp[0],
                      h->ldT, h->err_flag, h->kn.wt, (unsigned)((size_t)h->ldT * h->Dp[0] * ts(h)), (unsigned)((size_t)h->ldT * h->F * h->rw * 4), c.wts};
}

// layer 0: the gather of the batch's rows and their inner products -> a[0], aT[0]; training steps keep the raw embeddings (emb)
template <typename T> int ip_gather_fwd(ipnn_handle* h, const IpCall& c)
{
    IpProf ps(h, "ip_fwd");
    const IpRows rows = ip_fwd_rows(h);
    const IpKernel k = ip_gather_fwd_sel<T>(rows, c.wts != nullptr, h->kn.ipf_nt);
    const float inv_keep = c.drop ? 1.0f / h->cfg.keep_prob : 1.0f;
    T *a0 = (T*)h->a[0], *a0T = (T*)h->aT[0];
    float* emb = c.train ? h->emb : nullptr;
    if (rows == IP_WIDE) {
        const IpWideArgs wa = ip_wide_args(h, c, c.mask0, inv_keep);
        IHK(h, ip_launch(k, c.Ba / IPW_EX, ipw_fwd_lds(h->F, h->rw), h->st, wa, a0, a0T, emb));
    } else if (rows == IP_MANY) {
        const IpManyArgs ma = ip_many_args(h, c, c.mask0, inv_keep);
        IHK(h, ip_launch(k, c.Ba / IPM_EX, ipm_fwd_lds(h->F), h->st, ma, a0, a0T, emb));
    } else {
        const IpFwdArgs fa = ip_fwd_args(h, c, c.mask0, inv_keep);
        IHK(h, ip_launch(k, c.Ba / 16, ip16_lds(h->F, h->Dp[0]), h->st, fa, a0, a0T, emb));
    }
    return FNN_OK;
}

// ------------------------------------------------------------------------------------------------------------------- the stack
// The epilogues of the stack's products, for the strip kernels (the tile stays in LDS) and for the GEMM launches (row_major: the
// result also goes to HBM row-major, for the next launch).
template <typename T> EpiIpFwd<T> ip_epi_fwd(const ipnn_handle* h, const IpCall& c, int t, bool row_major)         // a_t, t = 1..L
{
    return EpiIpFwd<T>{row_major ? (T*)h->a[t] : nullptr, h->Dp[t], (T*)h->aT[t], h->ldT, c.drop ? h->maskT[t] : nullptr,
                       c.drop ? 1.0f / h->cfg.keep_prob : 1.0f, h->cfg.act, h->d[t], c.B};
}
template <typename T> EpiIpOut<T> ip_epi_out(const ipnn_handle* h, const IpCall& c)
{
    const int L = h->L;
    return EpiIpOut<T>{c.train ? (T*)h->dl[L] : nullptr, h->Dp[L + 1], c.train ? (T*)h->dlT[L] : nullptr, h->ldT, c.train ? c.y : nullptr,
                       c.logits_out, h->loss_t, c.p_out, c.B, h->loss_mean ? 1.0f / (float)c.B : 1.0f};
}
template <typename T> EpiIpBwd<T> ip_epi_bwd(const ipnn_handle* h, const IpCall& c, int t, bool row_major)         // product t -> delta l_{t-1}
{
    const bool first = (t == 1);
    const float keep = h->cfg.keep_prob;
    return EpiIpBwd<T>{row_major && !first ? (T*)h->dl[t - 2] : nullptr, h->Dp[t - 1], first ? nullptr : (T*)h->dlT[t - 2], h->ldT,
                       first ? h->dz0 : nullptr, h->Dp[0], (const T*)h->aT[t - 1], c.drop ? h->maskT[t - 1] : nullptr, 1.0f / keep, keep,
                       h->cfg.act, h->d[t - 1], c.B, first ? h->ref0 : nullptr};
}

// The pair state of one strip launch.  A launch of whole strips (the whole stack, or its wide products) takes the next epoch, pairs
// or not: the flags hold epoch * 16 + swap index, so every launch that could swap needs a number of its own, in launch order.  The
// 16-example tail never swaps and takes none.
StripDuo ip_strip_duo(ipnn_handle* h, bool tail, bool on)
{
    if (tail) return StripDuo{0, nullptr, nullptr, 0, h->err_flag, 0, h->kn.duo_min};
    return StripDuo{on ? 1 : 0, h->duo_xch, h->duo_flags, ++h->duo_epoch, h->err_flag, h->duo_xch_wg, h->kn.duo_min};
}

// the pairs' exchange buffers (made by the first call that runs pairs) and the epoch's wrap
template <typename T> int ip_duo_ready(ipnn_handle* h)
{
    constexpr int RT = sizeof(T) == 2 ? 2 : 1;
    const size_t nflags = (size_t)(h->ldT / (16 * RT)) * 2;
    if (!h->duo_xch) {
        h->duo_xch_wg = (size_t)2 * ((h->plan.maxD / 64 + 1) / 2) * RT * 256;       // 8-byte words: [2 parities][own blocks][RT][256]
        IHK(h, hipMalloc((void**)&h->duo_xch, nflags * h->duo_xch_wg * 8));
        IHK(h, hipMalloc((void**)&h->duo_flags, nflags * sizeof(int)));
        IHK(h, hipMemsetAsync(h->duo_flags, 0, nflags * sizeof(int), h->st));
    }
    if (h->duo_epoch >= (1 << 26)) {
        // flags hold epoch * 16 + swap index in 32 bits: long before that wraps (2^27 launches), drain the stream and start over at 0
        IHK(h, hipStreamSynchronize(h->st));
        IHK(h, hipMemsetAsync(h->duo_flags, 0, nflags * sizeof(int), h->st));
        h->duo_epoch = 0;
    }
    return FNN_OK;
}

// IPNN_TAIL_LDS=1: small products of a 16-example-strip launch whose weights go to LDS behind the tiles: each up to 64 KB, all of them
// within what is left of 152 KB.  Returns the bytes they take, fills the element offsets (-1: from memory).  OFF by default: measured
// (profiles/r03d_ipnn_tail_lds_ab.json) the 88 KB copy costs more than the k-steps it shortens.
template <typename T> size_t ip_tail_weights(const ipnn_handle* h, const int* Dp, int n, size_t tiles, int* wlds)
{
    const size_t budget = (size_t)152 * 1024 > tiles ? (size_t)152 * 1024 - tiles : 0;
    size_t used = 0;
    for (int p = 0; p < n; ++p) {
        const size_t b = (size_t)Dp[p] * Dp[p + 1] * sizeof(T);
        if (h->kn.tail_w_lds && b <= 64 * 1024 && used + b <= budget) { wlds[p] = (int)(used / sizeof(T)); used += b; }
        else wlds[p] = -1;
    }
    return used;
}

// Forward through the stack by the strip kernels: one launch, or (c.tsplit) the wide products 1 .. cut as pairs of 32-example
// strips, a[cut] through HBM, and the tail cut + 1 .. L + 1 as 16-example strips on every CU.  A fused tail is not launched here:
// its arguments go to the backward (*fused_tail).
// The whole stack as one strip launch, forward: everything but the pair state (duo), which is the launch site's.
template <typename T> StripFwdArgs<T> ip_stack_fwd_args(const ipnn_handle* h, const IpCall& c)
{
    const IpKnobs& kn = h->kn;
    const int L = h->L;
    StripFwdArgs<T> sa{};
    sa.a0 = (const T*)h->a[0]; sa.n = L + 1;
    for (int t = 0; t <= L + 1; ++t) sa.Dp[t] = h->Dp[t];
    for (int t = 1; t <= L + 1; ++t) sa.W[t - 1] = (const T*)h->wf[t - 1];
    for (int t = 1; t <= L; ++t) sa.ef[t - 1] = ip_epi_fwd<T>(h, c, t, false);
    sa.eo = ip_epi_out<T>(h, c);
    sa.dbg = h->stamps; sa.rot = kn.strip_rot; sa.sel = kn.stamp_sel;
    sa.has_out = 1; sa.finalF = nullptr; sa.warm = kn.strip_warm;
    for (int t = 0; t < STRIP_MAXP; ++t) sa.wlds[t] = -1;
    return sa;
}
// ... and backward
template <typename T> StripBwdArgs<T> ip_stack_bwd_args(const ipnn_handle* h, const IpCall& c)
{
    const IpKnobs& kn = h->kn;
    const int L = h->L;
    StripBwdArgs<T> sb{};
    sb.dlast = (const T*)h->dl[L]; sb.n = L + 1;
    for (int t = 0; t <= L + 1; ++t) sb.Dp[t] = h->Dp[t];
    for (int t = 1; t <= L + 1; ++t) { sb.W[t - 1] = (const T*)h->wb[t - 1]; sb.eb[t - 1] = ip_epi_bwd<T>(h, c, t, false); }
    sb.dbg = h->stamps ? h->stamps + (size_t)(h->ldT / 16) * 16 : nullptr; sb.rot = kn.strip_rot;
    sb.bottom = 1; sb.finalF = nullptr; sb.warm = kn.strip_warm;
    for (int t = 0; t < STRIP_MAXP; ++t) sb.wlds[t] = -1;
    return sb;
}

template <typename T> int ip_strips_fwd(ipnn_handle* h, const IpCall& c, StripFwdArgs<T>* fused_tail)
{
    IpProf ps(h, "fwd");
    const IpPlan& p = h->plan;
    const IpKnobs& kn = h->kn;
    const int L = h->L, cut = p.cut;
    constexpr int RT = sizeof(T) == 2 ? 2 : 1;
    StripFwdArgs<T> sa = ip_stack_fwd_args<T>(h, c);
    if (!c.tsplit) {
        sa.duo = ip_strip_duo(h, false, c.duo);
        IHK(h, ip_launch(ip_strip_sel<T>(false, RT, 4, STRIP_NW), c.nstrips * (c.duo ? 2 : 1), p.fwd.lds, h->st, sa, p.fwd.capA, p.fwd.capB));
        return FNN_OK;
    }
    StripFwdArgs<T> s1 = sa;                                  // products 1 .. cut: pairs of 32-example strips; a[cut] -> HBM
    s1.n = cut; s1.has_out = 0; s1.finalF = (T*)h->a[cut];
    s1.duo = ip_strip_duo(h, false, true);
    if (kn.stamps == 2) s1.dbg = nullptr;
    IHK(h, ip_launch(ip_strip_sel<T>(false, RT, kn.wide_nf, kn.wide_nw), c.nstrips * 2, p.wide_fwd.lds, h->st, s1, p.wide_fwd.capA, p.wide_fwd.capB));
    StripFwdArgs<T> s2{};                                     // products cut + 1 .. L + 1: 16-example strips, every CU
    s2.a0 = (const T*)h->a[cut]; s2.n = L + 1 - cut;
    for (int t = cut; t <= L + 1; ++t) s2.Dp[t - cut] = h->Dp[t];
    for (int t = cut + 1; t <= L + 1; ++t) s2.W[t - cut - 1] = sa.W[t - 1];
    for (int t = cut + 1; t <= L; ++t) s2.ef[t - cut - 1] = sa.ef[t - 1];
    s2.eo = sa.eo; s2.dbg = kn.stamps == 2 ? h->stamps : nullptr; s2.rot = kn.strip_rot; s2.sel = -1; s2.has_out = 1; s2.finalF = nullptr; s2.warm = sa.warm;
    s2.duo = ip_strip_duo(h, true, false);
    const size_t wl2 = ip_tail_weights<T>(h, s2.Dp, s2.n, p.tail_fwd.lds, s2.wlds);
    if (c.fuse_tail) *fused_tail = s2;
    else IHK(h, ip_launch(ip_strip_sel<T>(false, 1, kn.tail_nf, kn.tail_nw), c.Ba / 16, p.tail_fwd.lds + wl2, h->st, s2, p.tail_fwd.capA, p.tail_fwd.capB));
    return FNN_OK;
}

// Backward through the stack, the mirror image: the tail L + 1 .. cut + 1 first (with the forward tail in the same launch when
// fused), delta l_cut through HBM, then the wide products cut .. 1 as pairs.
template <typename T> int ip_strips_bwd(ipnn_handle* h, const IpCall& c, const StripFwdArgs<T>& fused_tail)
{
    IpProf ps(h, "bwd");
    const IpPlan& p = h->plan;
    const IpKnobs& kn = h->kn;
    const int L = h->L, cut = p.cut;
    constexpr int RT = sizeof(T) == 2 ? 2 : 1;
    StripBwdArgs<T> sb = ip_stack_bwd_args<T>(h, c);
    if (!c.tsplit) {
        sb.duo = ip_strip_duo(h, false, c.duo);
        IHK(h, ip_launch(ip_strip_sel<T>(true, RT, 4, STRIP_NW), c.nstrips * (c.duo ? 2 : 1), p.bwd.lds, h->st, sb, p.bwd.capA, p.bwd.capB));
        return FNN_OK;
    }
    StripBwdArgs<T> sA{};                                     // products L + 1 .. cut + 1 (the narrow ones come first): 16-example strips
    sA.dlast = (const T*)h->dl[L]; sA.n = L + 1 - cut;
    for (int t = cut; t <= L + 1; ++t) sA.Dp[t - cut] = h->Dp[t];
    for (int t = cut + 1; t <= L + 1; ++t) { sA.W[t - cut - 1] = sb.W[t - 1]; sA.eb[t - cut - 1] = sb.eb[t - 1]; }
    sA.dbg = kn.stamps == 2 ? sb.dbg : nullptr; sA.rot = kn.strip_rot; sA.bottom = 0; sA.finalF = (T*)h->dl[cut - 1]; sA.warm = sb.warm;
    sA.duo = ip_strip_duo(h, true, false);
    const size_t wlA = ip_tail_weights<T>(h, sA.Dp, sA.n, p.tail_bwd.lds, sA.wlds);
    if (c.fuse_tail) IHK(h, ip_launch(ip_strip_tail_sel<T>(), c.Ba / 16, p.tail.lds, h->st, fused_tail, sA, p.tail.capA, p.tail.capB));
    else IHK(h, ip_launch(ip_strip_sel<T>(true, 1, kn.tail_nf, kn.tail_nw), c.Ba / 16, p.tail_bwd.lds + wlA, h->st, sA, p.tail_bwd.capA, p.tail_bwd.capB));
    StripBwdArgs<T> sB = sb;                                  // products cut .. 1: pairs of 32-example strips, from delta l_cut in HBM
    sB.dlast = (const T*)h->dl[cut - 1]; sB.n = cut;
    if (kn.stamps == 2) sB.dbg = nullptr;
    sB.duo = ip_strip_duo(h, false, true);
    IHK(h, ip_launch(ip_strip_sel<T>(true, RT, kn.wide_nf, kn.wide_nw), c.nstrips * 2, p.wide_bwd.lds, h->st, sB, p.wide_bwd.capA, p.wide_bwd.capB));
    return FNN_OK;
}

// IPNN_STRIP=0, or a layer too wide for the strips' tiles: one product per launch, C [M][N] = A . B^T on fragment-tiled operands;
// narrow problems take smaller wave tiles
template <typename T, typename E>
void ip_gemm(ipnn_handle* h, const T* A, const T* Bm, int M, int N, int nkt_all, int nkt, int splitk, E epi)
{
    const int mt16 = M / 16, nt16 = N / 16;
    const long wg44 = (long)((M + 127) / 128) * ((N + 127) / 128) * splitk;
    const size_t lds4 = E::TILE ? gemm_ft_lds<T, 4>() : 0, lds2 = E::TILE ? gemm_ft_lds<T, 2>() : 0;
    if (wg44 >= 160 && h->kn.gemm_lds) {
        constexpr size_t ldsb = gemm_lds_bytes<T, E::TILE>();
        // > 64 KiB of dynamic LDS needs the opt-in (opt-in path: set on every launch, a host-side call)
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_lds<T, E>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsb);
        hipLaunchKernelGGL((k_gemm_lds<T, E>), dim3((M + 127) / 128, (N + 127) / 128, splitk), dim3(256), ldsb, h->st, A, Bm,
                           mt16, nt16, nkt_all, nkt, epi);
    } else if (wg44 >= 160)
        hipLaunchKernelGGL((k_gemm_ft<T, 4, 4, E>), dim3((M + 127) / 128, (N + 127) / 128, splitk), dim3(256), lds4, h->st, A, Bm,
                           mt16, nt16, nkt_all, nkt, epi);
    else if (N > 64)
        hipLaunchKernelGGL((k_gemm_ft<T, 2, 4, E>), dim3((M + 63) / 64, (N + 127) / 128, splitk), dim3(256), lds4, h->st, A, Bm,
                           mt16, nt16, nkt_all, nkt, epi);
    else
        hipLaunchKernelGGL((k_gemm_ft<T, 2, 2, E>), dim3((M + 63) / 64, (N + 63) / 64, splitk), dim3(256), lds2, h->st, A, Bm,
                           mt16, nt16, nkt_all, nkt, epi);
}
template <typename T> void ip_gemms_fwd(ipnn_handle* h, const IpCall& c)       // l_t = a_{t-1} W_t ; a_t = drop(act(l_t)); then the output unit
{
    IpProf ps(h, "fwd");
    constexpr int KS = Traits<T>::KS;
    for (int t = 1; t <= h->L + 1; ++t) {
        const T *A = (const T*)h->a[t - 1], *W = (const T*)h->wf[t - 1];
        const int nkt = h->Dp[t - 1] / KS;
        if (t <= h->L) ip_gemm(h, A, W, c.Ba, h->Dp[t], nkt, nkt, 1, ip_epi_fwd<T>(h, c, t, true));
        else ip_gemm(h, A, W, c.Ba, h->Dp[t], nkt, nkt, 1, ip_epi_out<T>(h, c));
    }
}
template <typename T> void ip_gemms_bwd(ipnn_handle* h, const IpCall& c)       // delta l_{t-1} from delta l_t
{
    IpProf ps(h, "bwd");
    constexpr int KS = Traits<T>::KS;
    for (int t = h->L + 1; t >= 1; --t)
        ip_gemm(h, (const T*)h->dl[t - 1], (const T*)h->wb[t - 1], c.Ba, h->Dp[t - 1], h->Dp[t] / KS, h->Dp[t] / KS, 1, ip_epi_bwd<T>(h, c, t, true));
}

// ------------------------------------------------------------------------------------------------------- after the backward pass
// The side chain: the backward of the inner products, b, the sparse-row update and (Adam / FTRL) the table pass.  They need dz1
// only; the weight gradients, beside them on the main stream, need the transposed operands only.
// the step size of the step that will be the handle's adam_t-th: Adam's bias-corrected lr_t, else lr
float ip_lr_step(const ipnn_handle* h, int64_t adam_t)
{
    if (!h->adam || h->ftrl) return h->cfg.lr;
    return (float)((double)h->cfg.lr * std::sqrt(1.0 - std::pow((double)h->cfg.adam_beta2, (double)adam_t)) /
                   (1.0 - std::pow((double)h->cfg.adam_beta1, (double)adam_t)));
}
// The argument blocks of the side chain, filled here for the solo launches and for the group step's records alike.
IpBwdArgs ip_bwd_args(const ipnn_handle* h, const IpCall& c)        // the 16-example backward of the inner products
{
    return IpBwdArgs{h->P, c.ids, c.B, h->F, h->K, h->table16, h->n_rows, h->Dp[0], h->emb, c.wts};
}
IpBArgs ip_b_args(const ipnn_handle* h, const IpCall& c, float lr_step)
{
    return IpBArgs{h->b, h->gb_part, c.Ba / ip_bwd_ex(h), h->adam ? (int)h->cfg.optimizer : 0, h->bmv, lr_step, h->cfg.adam_beta1,
                   h->cfg.adam_beta2, h->cfg.adam_eps, h->err_flag};
}
// sparse rows: row -= lr * sum of its gradients (c = 1: the table of powers is all ones).  Adam / FTRL: the same sorted sums
// land in the (zero) gradient table instead: G[row] = 0 * 1 - (-1) * sum.  Narrow rows: level 2 in the handle's form.
ScatArgs ip_scat_args(const ipnn_handle* h)
{
    ScatArgs sa = scat_args(h->rg, SORT_N, h->F, h->K, h->gxp, h->Dp[0], h->cpow1, h->adam ? -1.0 : (double)h->cfg.lr,
                            h->adam ? h->tG : h->table16, h->wide ? h->rw : SLOT);
    if (!h->wide) sa.form2 = h->kn.scat2_form;
    return sa;
}
void ip_b_update(const ipnn_handle* h, const IpCall& c, hipStream_t ss, float lr_step)
{
    const IpBArgs bu = ip_b_args(h, c, lr_step);                   // (ngb: one partial of db per workgroup of the backward)
    hipLaunchKernelGGL(k_ip_b_update, dim3(1), dim3(256), 0, ss, bu.b, bu.gb_part, bu.ngb, bu.opt, bu.bmv, bu.lr, bu.beta1, bu.beta2, bu.eps, bu.err);
}
void ip_adam_table(ipnn_handle* h, hipStream_t ss, float lr_step)
{
    const size_t n = (size_t)h->n_rows * h->rw;
    hipLaunchKernelGGL(k_adam_table, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, ss, h->table16, h->tm, h->tv, h->tG, n,
                       lr_step, h->cfg.adam_beta1, h->cfg.adam_beta2, h->cfg.adam_eps, (int)h->cfg.optimizer);
}

int ip_side_chain(ipnn_handle* h, const IpCall& c, hipStream_t ss, float lr_step)
{
    const int F = h->F;
    {
        IpProf ps(h, "ip_bwd", ss);
        const IpRows rows = ip_bwd_rows(h);
        const bool wv = c.wts != nullptr;
        const IpKernel k = ip_gather_bwd_sel(rows, wv);
        const float *dz0 = h->dz0, *emb = h->emb;
        if (rows == IP_WIDE) {
            const IpWideArgs wa = ip_wide_args(h, c, nullptr, 1.0f);
            IHK(h, ip_launch(k, c.Ba / IPW_EX, ipw_bwd_lds(F, h->rw, h->P, wv), ss, wa, dz0, emb, h->gxp, h->gb_part));
        } else if (rows == IP_MANY) {
            const IpManyArgs ma = ip_many_args(h, c, nullptr, 1.0f);
            IHK(h, ip_launch(k, c.Ba / IPM_BEX, ipm_bwd_lds(F, h->P, wv), ss, ma, dz0, emb, h->gxp, h->gb_part));
        } else {
            const IpBwdArgs ba = ip_bwd_args(h, c);
            IHK(h, ip_launch(k, c.Ba / 16, ip16_lds(F, h->Dp[0]), ss, ba, dz0, h->gxp, h->gb_part));
        }
        ip_b_update(h, c, ss, lr_step);
    }
    {
        IpProf ps(h, "scatter", ss);
        ScatArgs sa = ip_scat_args(h);
        if (h->wide) {   // the bag table's wide scatter, gradient stride rw, row pitch Dp0
            sa.tag_shared = h->noshare; sa.stamp = 1; sa.gxf = h->rw;
            const int nthr = F * (SORT_N / WCH) * (h->rw / 4);
            hipLaunchKernelGGL(k_ip_scatw1, dim3((nthr + 255) / 256), dim3(256), 0, ss, sa);
            hipLaunchKernelGGL(k_ip_scatw2, dim3(256), dim3(256), 0, ss, sa);
        } else launch_scat_narrow(ss, sa, h->kn.scat_form, 256);
    }
    if (h->adam) {
        IpProf ps(h, "adam_table", ss);
        ip_adam_table(h, ss, lr_step);
    }
    return FNN_OK;
}

// All weight gradients: gW_t [Dp_{t-1}][Dp_t] = a_{t-1}^T . delta l_t, contraction over the examples, into split-K slabs (the
// split chosen per layer so that every product fills the chip): one grouped launch, or one launch per product
// the grouped launch's arguments for a batch: the plan's, with every product's k-steps
template <typename T> GemmGroupArgs ip_wgrad_args(const ipnn_handle* h, const IpCall& c)
{
    GemmGroupArgs g = h->plan.group;
    for (int i = 0; i <= h->L; ++i) g.p[i].nkt = c.Ba / Traits<T>::KS / h->sk[h->plan.wg_order[i] - 1];
    return g;
}
// ... and the dense update's
IpUpdArgs ip_upd_args(const ipnn_handle* h, const IpCall& c, float lr_step)
{
    IpUpdArgs u = h->plan.upd;
    u.lr = lr_step; u.ngb = c.Ba / ip_bwd_ex(h); u.Ba = c.Ba;
    return u;
}
template <typename T> void ip_wgrad(ipnn_handle* h, const IpCall& c)
{
    IpProf ps(h, "wgrad");
    const IpPlan& p = h->plan;
    const int L = h->L;
    constexpr int KS = Traits<T>::KS;
    if (h->kn.group_wgrad && L + 1 <= GEMM_GROUP_MAX) {
        const GemmGroupArgs g = ip_wgrad_args<T>(h, c);
        hipLaunchKernelGGL((k_gemm_group<T, 4, 4>), dim3(g.wg0[L + 1]), dim3(256), gemm_f32w_lds(), h->st, g);
        return;
    }
    for (int t = 1; t <= L + 1; ++t) {
        const int sk = h->sk[t - 1];
        ip_gemm(h, (const T*)h->aT[t - 1], (const T*)h->dlT[t - 1], h->Dp[t - 1], h->Dp[t], h->ldT / KS, c.Ba / KS / sk, sk,
                EpiF32{h->slab + p.off[t - 1], h->Dp[t], h->slab_stride});
    }
}

// every dense layer's update from its slabs, b's, and the step's loss sum, in one launch
template <typename T> void ip_dense_update(ipnn_handle* h, const IpCall& c, hipStream_t us, float lr_step)
{
    IpProf ps(h, "update", us);
    const IpUpdArgs u = ip_upd_args(h, c, lr_step);
    hipLaunchKernelGGL((k_ip_update_all<T>), dim3((unsigned)(u.off[h->L + 1] / 4096 + 1)), dim3(256), 0, us, u);
}

// One forward pass (predict, eval) or one training step.  Everything that can refuse the call stands in front of the first enqueue.
template <typename T>
int ip_run(ipnn_handle* h, IpCall c)
{
    const IpPlan& p = h->plan;
    const IpKnobs& kn = h->kn;
    if (c.train && c.masks && !c.draw) for (int t = 0; t <= h->L; ++t) if (!c.masks[t]) IFAIL(h, FNN_ERR_ARG, "masks: null entry");
    ip_form(h, c);
    IpSide side(h);
    IRC(ip_join_table(h));                                      // the previous step's sparse rows / bias (read by the gather)
    if (c.train) {
        // beside the stack, on the side stream: the grouping of the batch's ids; the keep-masks (needed from the first product on)
        // go first, on the main stream
        IRC(side.fork(h->ev.fork));
        IRC(ip_masks(h, c, side));
        ip_sort_ids(h, c, side.s);
    }
    const bool mask_wait = c.drop && kn.mask_side;             // IPNN_MASK_SIDE=1: the masks come from the side stream
    if (mask_wait && c.draw) IRC(side.wait(h->ev.mask));        // the inner-product forward reads the drawn mask0
    IRC(ip_gather_fwd<T>(h, c));
    if (mask_wait && !c.draw) IRC(side.wait(h->ev.mask));       // the strips / GEMMs read the transposed masks
    IRC(ip_join(h));                                            // the previous step's dense update (read from here on)
    if (c.duo) IRC(ip_duo_ready<T>(h));
    StripFwdArgs<T> fused_tail{};
    if (p.strip) IRC(ip_strips_fwd<T>(h, c, &fused_tail)); else ip_gemms_fwd<T>(h, c);
    if (!c.train) { IHK(h, hipGetLastError()); return FNN_OK; }
    if (p.strip) IRC(ip_strips_bwd<T>(h, c, fused_tail)); else ip_gemms_bwd<T>(h, c);
    if (h->adam) h->adam_t += 1;
    const float lr_step = ip_lr_step(h, h->adam_t);
    // Beside the weight gradients, on the side stream (after the id grouping, in stream order): the side chain
    const bool side_upd = side.on() && kn.upd_side;
    IRC(side.fork(h->ev.bwd));
    IRC(ip_side_chain(h, c, side.s, lr_step));
    IRC(side.signal(side_upd ? h->ev.tab : h->ev.join));
    ip_wgrad<T>(h, c);
    if (side_upd) {
        // IPNN_UPDATE_SIDE=1: the dense update runs at the END of the side chain, behind the weight gradients, and the main stream
        // does NOT wait for it at the end of the step: the next call's mask transposition and gather -- which read neither the dense
        // weights nor the slabs -- run beside it, and the wait sits in front of the first product (ip_join; ip_join_table in front
        // of the gather).  Every other entry point joins first.
        IRC(side.fork(h->ev.wg));
        ip_dense_update<T>(h, c, side.s, lr_step);
        IRC(side.signal(h->ev.join));
        h->tab_pending = h->upd_pending = true;
    } else {
        ip_dense_update<T>(h, c, h->st, lr_step);
        IRC(side.wait(h->ev.join));                             // the step ends when the side chain has
    }
    side.settle();
    IHK(h, hipGetLastError());
    return FNN_OK;
}

// --------------------------------------------------------------------------------------------- many models on one feed
// ipnn_predict_multi / ipnn_eval_multi ("Evaluating many inner-product models").  The group of one call is
// a GroupCall (group_call.h), refusals without a usable hs[0] left with ipnn_last_error(NULL).  In front of the stream join
// every member's deferred dense update and sparse-row chain (IPNN_UPDATE_SIDE=1) join its own stream: ip_join.
struct IpGroup : GroupCall<ipnn_handle> {
    IpGroup(ipnn_handle* const* hs_, int n_, const char* name_) : GroupCall(name_, hs_, n_, IPNN_EVAL_MAX_MODELS, g_ip_err, ip_join) {}
};

// What both calls refuse, all of it before anything is launched or written.
int ip_group_check(const IpGroup& g, const int32_t* ids, bool need_y, const int32_t* y, int64_t N, bool need_p, float* const* p_out)
{
    IRC(g.check_list(nullptr));                                 // (the same handle twice: this family's own rule, below)
    ipnn_handle* const* hs = g.hs;
    const int M = g.n;
    if (!ids) return g.refuse(FNN_ERR_ARG, "null ids");
    if (need_y && !y) return g.refuse(FNN_ERR_ARG, "null y");
    if (need_p && !p_out) return g.refuse(FNN_ERR_ARG, "null p_out");
    if (need_p) for (int m = 0; m < M; ++m) if (!p_out[m]) return g.refuse(FNN_ERR_ARG, g.at("null p_out", m));
    if (N < 1 || N > ((int64_t)1 << 30)) return g.refuse(FNN_ERR_ARG, "N must be in [1, 2^30]");
    {   // A member's a[0] is the scratch of the group launch: no handle twice.  Not GroupCall::check_list's rule: this one comes
        // after the arguments' checks, names both places and reports the pair with the smallest second index.
        std::vector<std::pair<const ipnn_handle*, int>> v;
        for (int m = 0; m < M; ++m) v.emplace_back(hs[m], m);
        std::sort(v.begin(), v.end());
        int bi = -1, bj = -1;                                    // the pair with the smallest second index
        for (int i = 0; i + 1 < M; ++i)
            if (v[i].first == v[i + 1].first && (bj < 0 || v[i + 1].second < bj)) { bi = v[i].second; bj = v[i + 1].second; }
        if (bj >= 0) return g.refuse(FNN_ERR_ARG, g.at("the same handle as model " + std::to_string(bi) + " (a handle's own buffers are the group launch's scratch: list it once)", bj));
    }
    for (int m = 0; m < M; ++m) if (!hs[m]->table16) return g.refuse(FNN_ERR_STATE, g.at("ipnn_set_table has not been called", m));
    return FNN_OK;
}

// The members that one pair of group launches serves: a prediction LAUNCH CLASS -- element type, depth, padded widths, the
// gather's row kind (with its block size, and the row width of wide rows: they size its LDS), pairs, weights given or not.
// Activation, k, table size and every parameter value may differ inside a class.  members: positions in the list, in its order.
struct IpPredClass {
    bool bf16; int L; int Dp[STRIP_MAXP + 1]; IpRows rows; int nt, rw, P; bool wv; int capA, capB;      // capA, capB: the forward launch's tiles
    std::vector<int> members;
    bool same(const IpPredClass& o) const
    {
        if (bf16 != o.bf16 || L != o.L || rows != o.rows || nt != o.nt || rw != o.rw || P != o.P || wv != o.wv) return false;
        if (capA != o.capA || capB != o.capB) return false;
        for (int t = 0; t <= L + 1; ++t) if (Dp[t] != o.Dp[t]) return false;
        return true;
    }
};
IpPredClass ip_pred_class_of(const ipnn_handle* h, bool wv)
{
    IpPredClass c{};
    c.bf16 = h->bf16; c.L = h->L; c.rows = ip_fwd_rows(h); c.nt = c.rows == IP_NARROW ? h->kn.ipf_nt : 256; c.rw = h->rw; c.P = h->P; c.wv = wv;
    c.capA = h->plan.fwd.capA; c.capB = h->plan.fwd.capB;
    for (int t = 0; t <= h->L + 1; ++t) c.Dp[t] = h->Dp[t];
    return c;
}
// a member's arguments of both group launches for one feed batch (c: the batch as a prediction call, formed)
template <typename T> void ip_fill_group_arg(const ipnn_handle* h, int model, const IpCall& c, void* dst)
{
    static_assert(sizeof(IpGroupArg<T>) == sizeof(IpGroupArg<float>), "one ring element for both element types");
    IpGroupArg<T> g{};
    g.err = h->err_flag; g.model = model; g.a0 = (T*)h->a[0];
    const IpRows rows = ip_fwd_rows(h);
    if (rows == IP_WIDE) g.w = ip_wide_args(h, c, nullptr, 1.0f);
    else if (rows == IP_MANY) g.m = ip_many_args(h, c, nullptr, 1.0f);
    else g.f = ip_fwd_args(h, c, nullptr, 1.0f);
    StripFwdArgs<T>& sa = g.s;
    const int L = h->L;
    sa.a0 = (const T*)h->a[0]; sa.n = L + 1;
    for (int t = 0; t <= L + 1; ++t) sa.Dp[t] = h->Dp[t];
    for (int t = 1; t <= L + 1; ++t) sa.W[t - 1] = (const T*)h->wf[t - 1];
    for (int t = 1; t <= L; ++t) { sa.ef[t - 1] = ip_epi_fwd<T>(h, c, t, false); sa.ef[t - 1].outT = nullptr; }   // nobody reads a prediction's transposed activations
    sa.eo = ip_epi_out<T>(h, c);
    sa.dbg = nullptr; sa.rot = h->kn.strip_rot; sa.sel = -1; sa.has_out = 1; sa.finalF = nullptr; sa.warm = 0;
    for (int t = 0; t < STRIP_MAXP; ++t) sa.wlds[t] = -1;
    sa.duo = StripDuo{0, nullptr, nullptr, 0, h->err_flag, 0, h->kn.duo_min};
    memcpy(dst, &g, sizeof(g));
}
// one class's two launches for a feed batch of Ba padded lines: the gather with its inner products, then the whole stack
template <typename T> hipError_t ip_launch_class(const ipnn_handle* h, const IpPredClass& c, const void* dev_args, int Ba, hipStream_t st)
{
    constexpr int RT = sizeof(T) == 2 ? 2 : 1;
    const IpGroupArg<T>* d = static_cast<const IpGroupArg<T>*>(dev_args);
    const unsigned M = (unsigned)c.members.size();
    const int ex = c.rows == IP_WIDE ? IPW_EX : c.rows == IP_MANY ? IPM_EX : 16;
    const size_t lds = c.rows == IP_WIDE ? ipw_fwd_lds(h->F, h->rw) : c.rows == IP_MANY ? ipm_fwd_lds(h->F) : ip16_lds(h->F, h->Dp[0]);
    hipError_t e = ip_launch(ip_gather_fwd_g_sel<T>(c.rows, c.wv, c.nt), dim3((unsigned)(Ba / ex), M), lds, st, d);
    if (e != hipSuccess) return e;
    const IpTiles& tl = h->plan.fwd;
    return ip_launch(ip_strip_g_sel<T>(), dim3((unsigned)(Ba / (16 * RT)), M), tl.lds, st, d, tl.capA, tl.capB);
}

// The predictions of the n members hs[0 .. n) of group `g` (positions base .. in the call) on the N lines, p[m] each.  Members on
// the strip kernels: per feed batch -- as many lines as the smallest member's buffers hold, at most 4096, a multiple of 256 --
// their arguments through hs[0]'s ring and two launches per launch class.  Then the members off the strips (a layer too wide for
// the tiles, IPNN_STRIP=0), one after the other in chunks of their own max_batch, their stream swapped for the group's.
// (all_own: every member runs its own launches -- a single model, whose solo forms fill the chip better than one model's strips)
int ip_group_forward(const IpGroup& g, ipnn_handle* const* hs, int n, int base, const int32_t* ids, const float* wts, int64_t N, float* const* p,
                     bool all_own = false)
{
    ipnn_handle* h0 = g.h0;
    const hipStream_t st = h0->st;
    const int F = h0->F;
    std::vector<IpPredClass> cls;
    std::vector<int> own;
    int fb = 4096, ng = 0;
    for (int m = 0; m < n; ++m) {
        if (all_own || !hs[m]->plan.strip) { own.push_back(m); continue; }
        cls[class_index(cls, ip_pred_class_of(hs[m], wts != nullptr))].members.push_back(m);
        fb = std::min(fb, hs[m]->ldT); ++ng;
    }
    const size_t elem = h0->eval_ring.elem;
    for (int64_t lo = 0; ng && lo < N; lo += fb) {
        const int B = (int)std::min<int64_t>(fb, N - lo);
        size_t slot = 0;
        IHK(h0, ring_take(h0->eval_ring, (size_t)ng, &slot));
        char* a = h0->eval_ring.host_bytes(slot);
        const char* d = h0->eval_ring.dev_bytes(slot);
        size_t pos = 0;
        int Ba = 0;
        for (const IpPredClass& c : cls) for (int m : c.members) {
            ipnn_handle* h = hs[m];
            IpCall call{ids + lo * F, wts ? wts + lo * F : nullptr, nullptr, B, nullptr, nullptr, nullptr, p[m] + lo, false};
            ip_form(h, call);
            Ba = call.Ba;
            if (h->bf16) ip_fill_group_arg<bf16_t>(h, base + m, call, a + pos * elem); else ip_fill_group_arg<float>(h, base + m, call, a + pos * elem);
            ++pos;
        }
        IHK(h0, ring_send(h0->eval_ring, slot, (size_t)ng, st));
        pos = 0;
        for (const IpPredClass& c : cls) {
            const ipnn_handle* h = hs[c.members[0]];
            IHK(h0, c.bf16 ? ip_launch_class<bf16_t>(h, c, d + pos * elem, Ba, st) : ip_launch_class<float>(h, c, d + pos * elem, Ba, st));
            pos += c.members.size();
        }
    }
    IHK(h0, hipGetLastError());
    for (int m : own) {
        ipnn_handle* h = hs[m];
        const int rc = on_stream(h, st, [&] {
            int r = FNN_OK;
            for (int64_t lo = 0; r == FNN_OK && lo < N; lo += h->Bmax) {
                const int B = (int)std::min<int64_t>(h->Bmax, N - lo);
                const IpCall call{ids + lo * F, wts ? wts + lo * F : nullptr, nullptr, B, nullptr, nullptr, nullptr, p[m] + lo, false};
                r = h->bf16 ? ip_run<bf16_t>(h, call) : ip_run<float>(h, call);
            }
            return r;
        });
        if (rc != FNN_OK) return g.member_failed(rc, h, base + m);
    }
    return FNN_OK;
}

// --------------------------------------------------------------------------------------------- many models, one mini-batch step
// ipnn_train_step_multi ("A mini-batch step for many inner-product models").
struct IpStepGroup : GroupCall<ipnn_handle> {
    IpStepGroup(ipnn_handle* const* hs_, int n_) : GroupCall("ipnn_train_step_multi", hs_, n_, IPNN_STEP_MAX_MODELS, g_ip_err, ip_join) {}
};
// A member shares the group launches when its plan says so (ip_shares_step) and its segments are not being timed.
bool ip_step_shares(const ipnn_handle* h) { return ip_shares_step(h->plan, h->dims, h->kn) && !h->prof; }
// A training LAUNCH CLASS: the prediction launch class (element type, depth, padded widths, the gather's row kind and block size,
// pairs, weights given or not, the forward tiles), the row kind and the tiles of the backward, and the tiles of the grouped
// weight-gradient launch (the split-K of every product).  Everything else that
// differs between two members is a run-time field of their records: the scatter forms, wt, the optimiser, act, k, every value.
// Its members are pc.members.
struct IpStepClass {
    IpPredClass pc; int n_wg; IpRows rows_bwd; int capA_bwd, capB_bwd;
    bool same(const IpStepClass& o) const
    {
        return pc.same(o.pc) && n_wg == o.n_wg && rows_bwd == o.rows_bwd && capA_bwd == o.capA_bwd && capB_bwd == o.capB_bwd;
    }
};
// A GROUPING CLASS: members whose sparse-row updates read one grouping of the batch's ids -- the same keys (n_rows, key width)
// sorted the same way (runs) -- made once, in the first member's buffers.
struct IpSortClass { int64_t n_rows; bool key64; int merge4; ipnn_handle* first; };

// member m's call of one group step: its masks or its draw, formed as the single-strip form of the step
IpCall ip_step_call(const ipnn_handle* h, const int32_t* ids, const float* wts, const float* y, int B, const uint8_t* const* mk,
                    const IpDraw* dr, float* logits)
{
    IpCall c{ids, wts, y, B, mk, dr, logits, nullptr, true};
    ip_form(h, c);
    c.duo = c.tsplit = c.fuse_tail = false;
    return c;
}
template <typename T> void ip_fill_step_arg(ipnn_handle* h, int model, const IpCall& c, const int4* rec, float* pack, void* dst)
{
    IpStepArg<T> r{};
    const int L = h->L;
    r.model = model; r.pack = pack;
    r.drawn = c.draw ? 1 : 0;
    if (c.drop && c.draw) r.md = ip_step_draw_args(h, c, &r.n_mask);
    else if (c.drop) r.mt = ip_step_maskT_args(h, c, &r.n_mask);
    const float inv_keep = c.drop ? 1.0f / h->cfg.keep_prob : 1.0f;
    if (ip_fwd_rows(h) == IP_NARROW) r.f = ip_fwd_args(h, c, c.mask0, inv_keep);
    if (ip_fwd_rows(h) == IP_MANY || ip_bwd_rows(h) == IP_MANY) r.m = ip_many_args(h, c, c.mask0, inv_keep);      // (the backward reads neither the mask nor inv_keep)
    r.a0 = (T*)h->a[0]; r.a0T = (T*)h->aT[0]; r.emb = h->emb;
    const StripDuo solo{0, nullptr, nullptr, 0, h->err_flag, 0, h->kn.duo_min};     // one workgroup per strip: nothing to wait for
    r.s = ip_stack_fwd_args<T>(h, c); r.s.duo = solo; r.s.warm = 0; r.s.dbg = nullptr; r.s.sel = -1;
    r.sb = ip_stack_bwd_args<T>(h, c); r.sb.duo = solo; r.sb.warm = 0; r.sb.dbg = nullptr;
    if (ip_bwd_rows(h) == IP_NARROW) r.ib = ip_bwd_args(h, c);
    r.dz0 = h->dz0; r.gxp = h->gxp; r.gb_part = h->gb_part;
    const float lr_step = ip_lr_step(h, h->adam_t + (h->adam ? 1 : 0));
    r.bu = ip_b_args(h, c, lr_step);
    r.sa = ip_scat_args(h); r.sa.rec = rec;
    r.n_scat1 = scat1_blocks(r.sa, h->kn.scat_form);
    r.g = ip_wgrad_args<T>(h, c); r.n_wg = r.g.wg0[L + 1];
    r.u = ip_upd_args(h, c, lr_step);
    memcpy(dst, &r, sizeof(r));
}
// every stage of the step for one launch class, each ONE launch over (the stage's extent, the class's members); `d`: the members'
// records on the device.  ext: the largest extents among the members (mask tiles of either kind, level-1 workgroups).
struct IpStepExt { int n_draw = 0, n_maskT = 0, n_scat1 = 0; };
template <typename T> hipError_t ip_launch_step_class(const ipnn_handle* h, const IpStepClass& c, const IpStepExt& x, const void* dev_args,
                                                       int Ba, hipStream_t st)
{
    constexpr int RT = sizeof(T) == 2 ? 2 : 1;
    const IpStepArg<T>* d = static_cast<const IpStepArg<T>*>(dev_args);
    const unsigned M = (unsigned)c.pc.members.size();
    // the inner-product layer by row kind, per direction: examples per workgroup (the grid's unit) and dynamic LDS
    const bool many_f = c.pc.rows == IP_MANY, many_b = c.rows_bwd == IP_MANY;
    const int ex_f = many_f ? IPM_EX : 16, ex_b = many_b ? IPM_BEX : 16;
    const size_t lds_f = many_f ? ipm_fwd_lds(h->F) : ip16_lds(h->F, h->Dp[0]);
    const size_t lds_b = many_b ? ipm_bwd_lds(h->F, h->P, c.pc.wv) : ip16_lds(h->F, h->Dp[0]);
    const IpTiles &tf = h->plan.fwd, &tb = h->plan.bwd;
    hipError_t e = hipSuccess;
#define STEP_K(expr) do { if ((e = (expr)) != hipSuccess) return e; } while (0)
    if (x.n_draw) STEP_K(ip_launch(IP_K(256, k_mask_draw_g<T>), dim3((unsigned)x.n_draw, M), 0, st, d));
    if (x.n_maskT) STEP_K(ip_launch(IP_K(256, k_mask_T_g<T>), dim3((unsigned)x.n_maskT, M), 0, st, d));
    STEP_K(ip_launch(ip_step_gather_sel<T>(c.pc.rows, c.pc.wv, c.pc.nt), dim3((unsigned)(Ba / ex_f), M), lds_f, st, d));
    STEP_K(ip_launch(ip_step_strip_sel<T>(false), dim3((unsigned)(Ba / (16 * RT)), M), tf.lds, st, d, tf.capA, tf.capB));
    STEP_K(ip_launch(ip_step_strip_sel<T>(true), dim3((unsigned)(Ba / (16 * RT)), M), tb.lds, st, d, tb.capA, tb.capB));
    STEP_K(ip_launch(ip_step_bwd_sel<T>(c.rows_bwd, c.pc.wv), dim3((unsigned)(Ba / ex_b), M), lds_b, st, d));
    STEP_K(ip_launch(IP_K(256, k_ip_b_update_g<T>), dim3(M), 0, st, d));
    STEP_K(ip_launch(IP_K(256, k_ip_scat1_g<T>), dim3((unsigned)x.n_scat1, M), 0, st, d));
    STEP_K(ip_launch(IP_K(256, k_ip_scat2_g<T>), dim3(256, M), 0, st, d));
    STEP_K(ip_launch(IP_K(256, k_ip_wgrad_g<T>), dim3((unsigned)c.n_wg, M), gemm_f32w_lds(), st, d));
    STEP_K(ip_launch(IP_K(256, k_ip_update_all_g<T>), dim3((unsigned)(h->plan.upd.off[h->L + 1] / 4096 + 1), M), 0, st, d));
#undef STEP_K
    return hipSuccess;
}

// one solo training step of h, as ipnn_train_step_w / ipnn_train_step_drawn enqueue it (no loss copy, no synchronisation)
int ip_step_enqueue(ipnn_handle* h, const int32_t* ids, const float* wts, const float* y, int B, const uint8_t* const* masks, const IpDraw* draw,
                    float* logits_out)
{
    if (draw && !h->mask0) IHK(h, hipMalloc((void**)&h->mask0, (size_t)h->Bmax * h->d[0]));      // every byte a step reads is drawn by that step
    const IpCall c{ids, wts, y, B, masks, draw, logits_out, nullptr, true};
    return h->bf16 ? ip_run<bf16_t>(h, c) : ip_run<float>(h, c);
}

}  // namespace

extern "C" {

const char* ipnn_last_error(const ipnn_handle* h) { return h ? h->err.c_str() : g_ip_err.c_str(); }

uint64_t ipnn_cfg_size(void) { return (uint64_t)sizeof(ipnn_cfg); }

uint64_t ipnn_plan_info_size(void) { return (uint64_t)sizeof(ipnn_plan_info); }

// what ipnn_create would choose: its own check, knobs, shape and strip plan, with no device in between
int ipnn_plan_query(const ipnn_cfg* cfg, ipnn_plan_info* out)
{
    if (!cfg || !out) { g_ip_err = "null argument"; return FNN_ERR_ARG; }
    IRC(ip_cfg_check(cfg));
    const IpKnobs kn = ip_read_knobs();
    const IpDims dm = ip_dims(*cfg);
    const IpStrips p = ip_strip_plan(dm, kn);
    ipnn_plan_info o{};
    o.strips = p.strip; o.pairs = p.pairs; o.cut = p.cut;
    o.rows_fwd = dm.wide ? IPNN_ROWS_WIDE : dm.many_fwd ? IPNN_ROWS_MANY : IPNN_ROWS_NARROW;
    o.rows_bwd = dm.wide ? IPNN_ROWS_WIDE : dm.many_bwd ? IPNN_ROWS_MANY : IPNN_ROWS_NARROW;
    o.shares_step = ip_shares_step(p, dm, kn); o.shares_eval = p.strip;
    o.n_layers = dm.L + 2;
    for (int t = 0; t <= dm.L + 1; ++t) o.padded[t] = dm.Dp[t];
    const struct { const IpTiles* t; ipnn_tiles* o; } tiles[] = {{&p.fwd, &o.stack_fwd}, {&p.bwd, &o.stack_bwd}, {&p.wide_fwd, &o.wide_fwd},
        {&p.wide_bwd, &o.wide_bwd}, {&p.tail_fwd, &o.tail_fwd}, {&p.tail_bwd, &o.tail_bwd}, {&p.tail, &o.tail_fused}};
    for (const auto& e : tiles) { *e.o = ipnn_tiles{e.t->capA, e.t->capB, (uint64_t)e.t->lds}; o.lds_max = std::max(o.lds_max, (uint64_t)e.t->lds); }
    *out = o;
    return FNN_OK;
}

int ipnn_create(const ipnn_cfg* cfg, ipnn_handle** out)
{
    if (!cfg || !out) { g_ip_err = "null argument"; return FNN_ERR_ARG; }
    *out = nullptr;
    IRC(ip_cfg_check(cfg));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_ip_err = "no HIP device (libfnn_hip.so has no CPU fallback)"; return FNN_ERR_HIP; }
    ipnn_handle* h = new ipnn_handle();
    h->cfg = *cfg; h->dev = cfg->device;
    h->kn = ip_read_knobs();
    const IpDims& dm = h->dims = ip_dims(*cfg);
    h->F = dm.F; h->K = dm.K; h->L = dm.L; h->wide = dm.wide; h->rw = dm.rw; h->P = dm.P; h->CB = dm.CB; h->bf16 = dm.bf16;
    h->many_fwd = dm.many_fwd; h->many_bwd = dm.many_bwd;
    h->d.assign(dm.d, dm.d + dm.L + 2); h->Dp.assign(dm.Dp, dm.Dp + dm.L + 2);
    h->Bmax = cfg->max_batch; h->ldT = rup(h->Bmax, 256);
    { int ncu = 0; if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && ncu > 0) h->n_cu = ncu; }
    auto fail = [&](int code) { g_ip_err = h->err; ipnn_destroy(h); return code; };
#define IK(expr) do { hipError_t e2_ = (expr); if (e2_ != hipSuccess) { h->err = std::string(#expr) + ": " + hipGetErrorString(e2_); return fail(FNN_ERR_HIP); } } while (0)
    IK(hipSetDevice(h->dev));
    if (cfg->stream) h->st = (hipStream_t)cfg->stream; else { IK(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking)); h->own_stream = true; }
    if (h->kn.side_stream) {
        IK(hipStreamCreateWithFlags(&h->st2, hipStreamNonBlocking));
        for (hipEvent_t* e : {&h->ev.fork, &h->ev.bwd, &h->ev.wg, &h->ev.join, &h->ev.tab, &h->ev.mask}) IK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    h->sk.resize(h->L + 1);
    for (int t = 1; t <= h->L + 1; ++t) {                          // ~256 workgroups of 128 x 128 per product
        const int tiles = ((h->Dp[t - 1] + 127) / 128) * ((h->Dp[t] + 127) / 128);
        int sk = 1;
        while (sk < h->splitk && tiles * sk * 2 <= h->kn.wgrad_want) sk *= 2;
        h->sk[t - 1] = sk;
    }
    auto al = [&](void** p, size_t bytes) { hipError_t e = hipMalloc(p, bytes); if (e == hipSuccess) e = hipMemsetAsync(*p, 0, bytes, h->st); return e; };
    const size_t Ba = h->ldT, tsz = ts(h);
    size_t nw = 0;
    h->W.assign(h->L + 1, nullptr); h->wf.assign(h->L + 1, nullptr); h->wb.assign(h->L + 1, nullptr);
    h->a.assign(h->L + 1, nullptr); h->aT.assign(h->L + 1, nullptr); h->dl.assign(h->L + 1, nullptr); h->dlT.assign(h->L + 1, nullptr);
    for (int t = 1; t <= h->L + 1; ++t) {
        const size_t n = (size_t)h->Dp[t - 1] * h->Dp[t]; nw += n;
        IK(al((void**)&h->W[t - 1], n * 4)); IK(al(&h->wf[t - 1], n * tsz)); IK(al(&h->wb[t - 1], n * tsz));
        IK(al(&h->dl[t - 1], Ba * h->Dp[t] * tsz)); IK(al(&h->dlT[t - 1], Ba * h->Dp[t] * tsz));
    }
    for (int t = 0; t <= h->L; ++t) { IK(al(&h->a[t], Ba * h->Dp[t] * tsz)); IK(al(&h->aT[t], Ba * h->Dp[t] * tsz)); }
    h->ftrl = cfg->optimizer == IPNN_OPT_FTRL;
    h->adam = cfg->optimizer == IPNN_OPT_ADAM || h->ftrl;          // both: per-variable state + dense table pass
    if (h->adam) {
        h->Wm.assign(h->L + 1, nullptr); h->Wv.assign(h->L + 1, nullptr);
        for (int t = 1; t <= h->L + 1; ++t) {
            const size_t n = (size_t)h->Dp[t - 1] * h->Dp[t];
            IK(al((void**)&h->Wm[t - 1], n * 4)); IK(al((void**)&h->Wv[t - 1], n * 4));
        }
        IK(al((void**)&h->bmv, 8));
        if (ip_reset_dense_state(h) != FNN_OK) return fail(FNN_ERR_HIP);
    }
    h->maskT.assign(h->L + 1, nullptr);
    for (int t = 0; t <= h->L; ++t) IK(al((void**)&h->maskT[t], Ba * h->Dp[t]));
    h->slab_stride = nw;
    IK(al((void**)&h->slab, (size_t)h->splitk * nw * 4));
    IK(al((void**)&h->emb, Ba * h->F * h->rw * 4));
    IK(al((void**)&h->dz0, Ba * h->Dp[0] * 4)); IK(al((void**)&h->gxp, Ba * h->Dp[0] * 4));
    IK(al((void**)&h->gb_part, (Ba / ip_bwd_ex(h)) * 4)); IK(al((void**)&h->loss_t, Ba * 4)); IK(al((void**)&h->loss_dev, 4));
    IK(al((void**)&h->b, 4)); IK(al((void**)&h->err_flag, 4));
    IK(row_group_alloc(h->rg, h->F, SORT_N, h->wide, h->wide ? h->rw : SLOT, h->st, /*owners16*/ true));
    IK(al(&h->skeys, (size_t)h->F * SORT_N * 8));
    {   // c = 1: every power is 1
        std::vector<double> ones(SORT_N + 1, 1.0);
        IK(hipMalloc((void**)&h->cpow1, ones.size() * 8));
        IK(hipMemcpy(h->cpow1, ones.data(), ones.size() * 8, hipMemcpyHostToDevice));
        std::vector<int> ref(h->Dp[0], -1);                       // slot column -> reference z1 column
        for (int f = 0; f < h->F; ++f) for (int l = 0; l < h->K; ++l) ref[f * h->rw + l] = f * h->K + l;
        for (int n = 0; n < h->P; ++n) ref[h->F * h->rw + n] = h->F * h->K + n;
        ref[h->CB] = h->d[0] - 1;
        IK(hipMalloc((void**)&h->ref0, ref.size() * 4));
        IK(hipMemcpy(h->ref0, ref.data(), ref.size() * 4, hipMemcpyHostToDevice));
        if (h->many_fwd && h->P) {                                    // pair n -> (i, j), i < j, row-major: the column order of z1's products
            std::vector<unsigned short> pt;
            pt.reserve(h->P);
            for (int i = 0; i < h->F; ++i) for (int j = i + 1; j < h->F; ++j) pt.push_back((unsigned short)(i | (j << 8)));
            IK(hipMalloc((void**)&h->ptab, pt.size() * 2));
            IK(hipMemcpy(h->ptab, pt.data(), pt.size() * 2, hipMemcpyHostToDevice));
        }
    }
    if (h->kn.stamps) IK(al((void**)&h->stamps, (size_t)2 * (h->ldT / 16) * 16 * 8));
    if (h->bf16) ip_make_plan<bf16_t>(h); else ip_make_plan<float>(h);
    if ((h->bf16 ? ip_opt_in<bf16_t>(h) : ip_opt_in<float>(h)) != FNN_OK) return fail(FNN_ERR_HIP);
    IK(hipStreamSynchronize(h->st));
#undef IK
    *out = h;
    return FNN_OK;
}

int ipnn_destroy(ipnn_handle* h)
{
    if (!h) return FNN_ERR_ARG;
    hipSetDevice(h->dev);
    if (h->st) { ip_join(h); hipStreamSynchronize(h->st); }
    for (auto v : {&h->wf, &h->wb, &h->a, &h->aT, &h->dl, &h->dlT}) for (void* p : *v) if (p) hipFree(p);
    for (float* p : h->W) if (p) hipFree(p);
    for (uint8_t* p : h->maskT) if (p) hipFree(p);
    for (float* p : h->Wm) if (p) hipFree(p);
    for (float* p : h->Wv) if (p) hipFree(p);
    for (float* p : {h->tm, h->tv, h->tG, h->bmv}) if (p) hipFree(p);
    void* ptrs[] = {h->mask0, h->table16, h->noshare, h->b, h->emb, h->dz0, h->gxp, h->gb_part, h->loss_t, h->loss_dev, h->slab, h->ref0, h->ptab, h->err_flag,
                    h->skeys, h->cpow1, h->duo_xch, h->duo_flags};
    for (void* p : ptrs) if (p) hipFree(p);
    if (h->ev_scratch) hipFree(h->ev_scratch);
    ring_release(h->eval_ring);
    ring_release(h->step_ring);
    if (h->step_pack) hipFree(h->step_pack);
    if (h->step_pack_host) hipHostFree(h->step_pack_host);
    if (h->join) hipEventDestroy(h->join);
    row_group_free(h->rg);
    for (auto& kv : h->prof_ev) for (auto& p : kv.second) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
    if (h->st2) { hipStreamSynchronize(h->st2); hipStreamDestroy(h->st2); }
    for (hipEvent_t e : {h->ev.fork, h->ev.bwd, h->ev.wg, h->ev.join, h->ev.tab, h->ev.mask}) if (e) hipEventDestroy(e);
    if (h->own_stream && h->st) hipStreamDestroy(h->st);
    delete h;
    return FNN_OK;
}

int ipnn_sync(ipnn_handle* h)
{
    if (!h) return FNN_ERR_ARG;
    int flag = 0;
    IRC(ip_join(h));
    IHK(h, hipMemcpyAsync(&flag, h->err_flag, 4, hipMemcpyDeviceToHost, h->st));
    IHK(h, hipStreamSynchronize(h->st));
    if (flag) {
        IHK(h, hipMemsetAsync(h->err_flag, 0, 4, h->st));
        if (flag & 2) {
            h->duo_failed = true;
            IFAIL(h, FNN_ERR_HIP, "a strip workgroup gave up waiting for its partner (StripDuo swap): that step's outputs are invalid and its dense update was not applied; the handle refuses further train steps (IPNN_STRIP_DUO=0 selects one workgroup per strip)");
        }
        IFAIL(h, FNN_ERR_RANGE, "feature id outside [0, n_rows)");
    }
    return FNN_OK;
}

int ipnn_set_table(ipnn_handle* h, const float* rows, int64_t n_rows)
{
    if (!h || !rows || n_rows < 1) return FNN_ERR_ARG;
    IHK(h, hipSetDevice(h->dev));
    IRC(ip_join(h));
    IHK(h, hipStreamSynchronize(h->st));
    if (h->table16) hipFree(h->table16);
    IHK(h, hipMalloc((void**)&h->table16, (size_t)n_rows * h->rw * 4));
    if (h->wide) {
        if (h->noshare) hipFree(h->noshare);
        h->noshare = nullptr;
        IHK(h, hipMalloc((void**)&h->noshare, (size_t)n_rows * 4));
        IHK(h, hipMemset(h->noshare, 0, (size_t)n_rows * 4));
    }
    float* tmp = nullptr;
    IHK(h, hipMalloc((void**)&tmp, (size_t)n_rows * h->K * 4));
    IHK(h, hipMemcpy(tmp, rows, (size_t)n_rows * h->K * 4, hipMemcpyHostToDevice));
    const size_t n = (size_t)n_rows * h->rw;
    hipLaunchKernelGGL(k_pack_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, tmp, n_rows, h->K, h->rw, h->table16);
    IHK(h, hipStreamSynchronize(h->st));
    hipFree(tmp);
    h->n_rows = n_rows;
    h->key64 = (unsigned long long)n_rows * SORT_N > 0xFFFFFFFFull;
    if (h->adam) {                                              // fresh moments and gradient table for the new rows
        for (float** p : {&h->tm, &h->tv, &h->tG}) {
            if (*p) { hipFree(*p); *p = nullptr; }
            IHK(h, hipMalloc((void**)p, n * 4));
            IHK(h, hipMemset(*p, 0, n * 4));
        }
        if (h->ftrl) hipLaunchKernelGGL(k_fill_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->tm, n, 0.1f);
        // the optimiser restarts as a whole (as fm_set_table does): every dense layer's and b's state as ipnn_create left them
        IRC(ip_reset_dense_state(h));
        IHK(h, hipStreamSynchronize(h->st));
    }
    return FNN_OK;
}

int ipnn_get_rows(ipnn_handle* h, const int64_t* row_ids, int64_t n, float* out)
{
    if (!h || !row_ids || !out || n < 1 || !h->table16) return FNN_ERR_ARG;
    IHK(h, hipSetDevice(h->dev));
    IRC(ip_join(h));
    int64_t* di = nullptr; float* dout = nullptr;
    IHK(h, hipMalloc((void**)&di, n * 8)); IHK(h, hipMalloc((void**)&dout, n * h->K * 4));
    IHK(h, hipMemcpy(di, row_ids, n * 8, hipMemcpyHostToDevice));
    const size_t cnt = (size_t)n * h->K;
    hipLaunchKernelGGL(k_unpack_rows, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, h->st, h->table16, di, n, h->n_rows, h->K, h->rw,
                       dout, h->err_flag);
    IHK(h, hipMemcpyAsync(out, dout, cnt * 4, hipMemcpyDeviceToHost, h->st));
    IHK(h, hipStreamSynchronize(h->st));
    hipFree(di); hipFree(dout);
    return FNN_OK;
}

int ipnn_set_b(ipnn_handle* h, float b)
{
    if (!h) return FNN_ERR_ARG;
    IHK(h, hipSetDevice(h->dev));
    IRC(ip_join(h));
    IHK(h, hipStreamSynchronize(h->st));
    IHK(h, hipMemcpy(h->b, &b, 4, hipMemcpyHostToDevice));
    return FNN_OK;
}
int ipnn_get_b(ipnn_handle* h, float* b)
{
    if (!h || !b) return FNN_ERR_ARG;
    IHK(h, hipSetDevice(h->dev));
    IRC(ip_join(h));
    IHK(h, hipStreamSynchronize(h->st));
    IHK(h, hipMemcpy(b, h->b, 4, hipMemcpyDeviceToHost));
    return FNN_OK;
}

// reference row r of layer `layer` -> padded row
static int ip_row_of(const ipnn_handle* h, int layer, int r)
{
    if (layer > 1) return r;
    const int FK = h->F * h->K;
    if (r < FK) return (r / h->K) * h->rw + r % h->K;
    if (r < FK + h->P) return h->F * h->rw + (r - FK);
    return h->CB;
}

int ipnn_set_layer(ipnn_handle* h, int layer, const float* W, const float* bias)
{
    if (!h || !W || !bias || layer < 1 || layer > h->L + 1) return FNN_ERR_ARG;
    IHK(h, hipSetDevice(h->dev));
    const int din = h->d[layer - 1], dout = h->d[layer], Din = h->Dp[layer - 1], Dout = h->Dp[layer];
    std::vector<float> p((size_t)Din * Dout, 0.f);
    for (int r = 0; r < din; ++r) memcpy(&p[(size_t)ip_row_of(h, layer, r) * Dout], &W[(size_t)r * dout], (size_t)dout * 4);
    const int ones_row = layer == 1 ? h->CB + 1 : din;
    memcpy(&p[(size_t)ones_row * Dout], bias, (size_t)dout * 4);
    IRC(ip_join(h));
    IHK(h, hipStreamSynchronize(h->st));
    IHK(h, hipMemcpy(h->W[layer - 1], p.data(), p.size() * 4, hipMemcpyHostToDevice));
    if (h->bf16) ip_refresh<bf16_t>(h, layer, nullptr, 0.f); else ip_refresh<float>(h, layer, nullptr, 0.f);
    IHK(h, hipStreamSynchronize(h->st));
    return FNN_OK;
}

int ipnn_get_layer(ipnn_handle* h, int layer, float* W, float* bias)
{
    if (!h || !W || !bias || layer < 1 || layer > h->L + 1) return FNN_ERR_ARG;
    IHK(h, hipSetDevice(h->dev));
    const int din = h->d[layer - 1], dout = h->d[layer], Din = h->Dp[layer - 1], Dout = h->Dp[layer];
    std::vector<float> p((size_t)Din * Dout);
    IRC(ip_join(h));
    IHK(h, hipStreamSynchronize(h->st));
    IHK(h, hipMemcpy(p.data(), h->W[layer - 1], p.size() * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < din; ++r) memcpy(&W[(size_t)r * dout], &p[(size_t)ip_row_of(h, layer, r) * Dout], (size_t)dout * 4);
    const int ones_row = layer == 1 ? h->CB + 1 : din;
    memcpy(bias, &p[(size_t)ones_row * Dout], (size_t)dout * 4);
    return FNN_OK;
}

int ipnn_train_step(ipnn_handle* h, const int32_t* ids, const float* y, int B, const uint8_t* const* masks,
                    float* logits_out, float* loss_sum_out)
{
    return ipnn_train_step_w(h, ids, nullptr, y, B, masks, logits_out, loss_sum_out);
}

// one training step: the caller's masks, the library's draw, or neither
static int ip_train_step(ipnn_handle* h, const int32_t* ids, const float* wts, const float* y, int B, const uint8_t* const* masks,
                         const IpDraw* draw, float* logits_out, float* loss_sum_out)
{
    if (!h || !ids || !y) return FNN_ERR_ARG;
    if (B < 1 || B > h->Bmax) IFAIL(h, FNN_ERR_ARG, "B must be in [1, max_batch]");
    if (!h->table16) IFAIL(h, FNN_ERR_STATE, "ipnn_set_table has not been called");
    if (h->duo_failed) IFAIL(h, FNN_ERR_STATE, "an earlier step failed (StripDuo swap timed out): re-create the handle");
    IHK(h, hipSetDevice(h->dev));
    IRC(ip_step_enqueue(h, ids, wts, y, B, masks, draw, logits_out));
    if (loss_sum_out) {                                      // (the loss is summed in the update launch: join it)
        IRC(ip_join(h));
        IHK(h, hipMemcpyAsync(loss_sum_out, h->loss_dev, 4, hipMemcpyDeviceToHost, h->st));
        return ipnn_sync(h);
    }
    return FNN_OK;
}

int ipnn_train_step_w(ipnn_handle* h, const int32_t* ids, const float* wts, const float* y, int B, const uint8_t* const* masks,
                      float* logits_out, float* loss_sum_out)
{
    return ip_train_step(h, ids, wts, y, B, masks, nullptr, logits_out, loss_sum_out);
}

int ipnn_train_step_drawn(ipnn_handle* h, const int32_t* ids, const float* wts, const float* y, int B, uint64_t seed, uint64_t step,
                          float* logits_out, float* loss_sum_out)
{
    const IpDraw dr{seed, step};
    return ip_train_step(h, ids, wts, y, B, nullptr, &dr, logits_out, loss_sum_out);
}

int ipnn_draw_masks(ipnn_handle* h, uint64_t seed, uint64_t step, int B, uint8_t* const* masks_out)
{
    if (!h || !masks_out) return FNN_ERR_ARG;
    if (B < 1 || B > h->Bmax) IFAIL(h, FNN_ERR_ARG, "B must be in [1, max_batch]");
    IHK(h, hipSetDevice(h->dev));
    int tiles = 0;
    MaskDrawArgs da = ip_draw_args(h, IpDraw{seed, step}, B, &tiles);
    for (int t = 0; t <= h->L; ++t) da.dstR[t] = masks_out[t];               // row-major targets only (a NULL entry: that layer's tiles return)
    hipLaunchKernelGGL(k_mask_draw, dim3(tiles), dim3(256), 0, h->st, da);
    IHK(h, hipGetLastError());
    return FNN_OK;
}

int ipnn_set_loss_mean(ipnn_handle* h, int mean)
{
    if (!h) return FNN_ERR_ARG;
    h->loss_mean = mean != 0;
    return FNN_OK;
}

int ipnn_predict(ipnn_handle* h, const int32_t* ids, int B, float* p_out) { return ipnn_predict_w(h, ids, nullptr, B, p_out); }

int ipnn_predict_w(ipnn_handle* h, const int32_t* ids, const float* wts, int B, float* p_out)
{
    if (!h || !ids || !p_out) return FNN_ERR_ARG;
    if (B < 1 || B > h->Bmax) IFAIL(h, FNN_ERR_ARG, "B must be in [1, max_batch]");
    if (!h->table16) IFAIL(h, FNN_ERR_STATE, "ipnn_set_table has not been called");
    IHK(h, hipSetDevice(h->dev));
    const IpCall c{ids, wts, nullptr, B, nullptr, nullptr, nullptr, p_out, false};
    return h->bf16 ? ip_run<bf16_t>(h, c) : ip_run<float>(h, c);
}

int ipnn_eval(ipnn_handle* h, const int32_t* ids, const int32_t* y, int64_t N, double* auc, double* rmse, double* logloss)
{
    return ipnn_eval_w(h, ids, nullptr, y, N, auc, rmse, logloss);
}

// One handle's evaluation pass up to its metrics: the predictions in chunks of max_batch -- into p_keep (DEVICE, [N]) when given,
// else into a buffer of the call's own -- and device_metrics on them (*mrc: its verdict, -2 / -3 with *merr; -1 is returned here)
static int ip_eval_solo(ipnn_handle* h, const int32_t* ids, const float* wts, const int32_t* y, int64_t N, float* p_keep, double out[4],
                        int* mrc, std::string* merr)
{
    IHK(h, hipSetDevice(h->dev));
    float* p_d = p_keep;
    if (!p_d) IHK(h, hipMalloc((void**)&p_d, (size_t)N * 4));
    for (int64_t lo = 0; lo < N; lo += h->Bmax) {
        const int B = (int)(N - lo < h->Bmax ? N - lo : h->Bmax);
        const float* w = wts ? wts + lo * h->F : nullptr;        // the chunk's weights travel with its ids
        const IpCall c{ids + lo * h->F, w, nullptr, B, nullptr, nullptr, nullptr, p_d + lo, false};
        const int rc = h->bf16 ? ip_run<bf16_t>(h, c) : ip_run<float>(h, c);
        if (rc != FNN_OK) { if (!p_keep) hipFree(p_d); return rc; }
    }
    *mrc = device_metrics(h->st, p_d, y, N, out, *merr);
    if (!p_keep) hipFree(p_d);
    if (*mrc == -1) IFAIL(h, FNN_ERR_HIP, *merr);
    return FNN_OK;
}

int ipnn_eval_w(ipnn_handle* h, const int32_t* ids, const float* wts, const int32_t* y, int64_t N, double* auc, double* rmse, double* logloss)
{
    if (!h || !ids || !y || N < 1) return FNN_ERR_ARG;
    if (!h->table16) IFAIL(h, FNN_ERR_STATE, "ipnn_set_table has not been called");
    double out[4] = {0, 0, 0, 0};
    std::string merr;
    int mrc = 0;
    IRC(ip_eval_solo(h, ids, wts, y, N, nullptr, out, &mrc, &merr));
    if (auc) *auc = out[0];
    if (rmse) *rmse = out[1];
    if (logloss) *logloss = out[2];
    const int rc = ipnn_sync(h);
    if (rc != FNN_OK) return rc;
    if (mrc == -2 || mrc == -3) IFAIL(h, FNN_ERR_RANGE, merr);
    return FNN_OK;
}

// The predictions of several handles on one feed: per feed batch and prediction launch class two launches with the model as a
// grid dimension.  Nothing is allocated after hs[0]'s first group call, nothing synchronises; an id outside a member's table shows
// at that member's ipnn_sync.
int ipnn_predict_multi(ipnn_handle* const* hs, int n_models, const int32_t* ids, const float* wts, int64_t N, float* const* p_out)
{
    IpGroup g(hs, n_models, "ipnn_predict_multi");
    IRC(ip_group_check(g, ids, false, nullptr, N, true, p_out));
    IRC(g.enter());
    IRC(ip_group_forward(g, hs, n_models, 0, ids, wts, N, p_out, n_models == 1));
    return g.leave();
}

// ... and their metrics: the models in groups of as many as fit $IPNN_EVAL_SCRATCH_BYTES (read per call; default 2^30, one model
// at the least); per group the predictions, one metrics_multi pass over them, the range flags, one copy home, one synchronisation.
int ipnn_eval_multi(ipnn_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const int32_t* y, int64_t N,
                    double* auc, double* rmse, double* logloss, int* status, float* const* p_out)
{
    IpGroup g(hs, n_models, "ipnn_eval_multi");
    IRC(ip_group_check(g, ids, true, y, N, false, nullptr));
    ipnn_handle* h0 = g.h0;
    if (n_models == 1) {
        // one model: the solo evaluation (measured: the group path is not faster there -- profiles/ipnn_eval_multi_bench.json --
        // and the solo strip forms fill the chip better), reported as the group path reports
        double out[4] = {0, 0, 0, 0};
        std::string merr;
        int mrc = 0;
        IRC(ip_eval_solo(h0, ids, wts, y, N, p_out ? p_out[0] : nullptr, out, &mrc, &merr));
        const double nan = std::nan("");
        if (auc) auc[0] = (mrc == -2 || mrc == -3) ? nan : out[0];
        if (rmse) rmse[0] = mrc == -3 ? nan : out[1];
        if (logloss) logloss[0] = mrc == -3 ? nan : out[2];
        if (status) status[0] = mrc == -3 ? FNN_ERR_RANGE : FNN_OK;
        const int rc = ipnn_sync(h0);
        if (rc != FNN_OK && rc != FNN_ERR_RANGE) return rc;
        const std::string msg = eval_verdict(mrc == -3 ? "0" : "", rc == FNN_ERR_RANGE ? "0" : "", mrc == -2, "[0, n_rows)");
        return msg.empty() ? FNN_OK : g.refuse(FNN_ERR_RANGE, msg);
    }
    const int G = eval_group_size(n_models, N, "IPNN_EVAL_SCRATCH_BYTES");
    IRC(g.enter());
    const hipStream_t st = h0->st;
    const size_t need = EvalScratch::bytes(G, N);                     // hs[0]'s buffer, grown to the largest call so far
    if (h0->ev_scratch_bytes < need) {                                // (the last user of the old one, an earlier call, has synchronised)
        if (h0->ev_scratch) { hipFree(h0->ev_scratch); h0->ev_scratch = nullptr; h0->ev_scratch_bytes = 0; }
        IHK(h0, hipMalloc((void**)&h0->ev_scratch, need));
        h0->ev_scratch_bytes = need;
    }
    const size_t elem = h0->eval_ring.elem;
    const EvalForward forward = [&](int g0, int n, float* const* p) { return ip_group_forward(g, hs + g0, n, g0, ids, wts, N, p); };
    const EvalFlags flags = [&](int g0, int n, int* flags_d) {        // the members' range bits, read and cleared on the device
        size_t slot = 0;
        IHK(h0, ring_take(h0->eval_ring, (size_t)n, &slot));
        char* a = h0->eval_ring.host_bytes(slot);
        for (int m = 0; m < n; ++m) {
            IpGroupArg<float> fa{};
            fa.err = hs[g0 + m]->err_flag; fa.model = m;
            memcpy(a + (size_t)m * elem, &fa, sizeof(fa));
        }
        IHK(h0, ring_send(h0->eval_ring, slot, (size_t)n, st));
        hipLaunchKernelGGL(k_ip_gflags, dim3(1), dim3(256), 0, st, h0->eval_ring.dev_bytes(slot), elem, n, flags_d);
        IHK(h0, hipGetLastError());
        return FNN_OK;
    };
    EvalFound found;
    const int rc = eval_groups(st, n_models, G, y, N, h0->ev_scratch, forward, flags, EvalOut{auc, rmse, logloss, status, p_out}, found, h0->err);
    const int rj = g.leave();
    if (rc != FNN_OK) return rc;                                      // (eval_groups has drained the stream: the buffer is free for the next call)
    if (rj != FNN_OK) return rj;
    const std::string msg = eval_verdict(found.bad, found.range, found.n_pos, N, "[0, n_rows)");
    return msg.empty() ? FNN_OK : g.refuse(FNN_ERR_RANGE, msg);
}

// One training step of several handles on one feed.  Members on the group path (ip_step_shares): their records through hs[0]'s
// step ring, one sort per grouping class, then per launch class every stage once; the others run their own step on the group's
// stream.  What a member keeps of a step on the host (the step count) is written after the last launch was accepted.
int ipnn_train_step_multi(ipnn_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const float* y, int B,
                          const uint8_t* const* const* masks, const uint64_t* seeds, const uint64_t* steps,
                          float* const* logits_out, float* loss_sum_out)
{
    IpStepGroup g(hs, n_models);
    IRC(g.check_list("it is written to"));
    const int M = n_models;
    if (!ids) return g.refuse(FNN_ERR_ARG, "null ids");
    if (!y) return g.refuse(FNN_ERR_ARG, "null y");
    if (B < 1) return g.refuse(FNN_ERR_ARG, "B must be at least 1");
    for (int m = 0; m < M; ++m)
        if (B > hs[m]->Bmax) return g.refuse(FNN_ERR_ARG, g.at("B = " + std::to_string(B) + " is above its max_batch = " + std::to_string(hs[m]->Bmax), m));
    if (masks && seeds) return g.refuse(FNN_ERR_ARG, "masks and seeds both given: the caller's masks or the library's draw, not both");
    if (seeds && !steps) return g.refuse(FNN_ERR_ARG, "seeds without steps");
    if (steps && !seeds) return g.refuse(FNN_ERR_ARG, "steps without seeds");
    if (masks) for (int m = 0; m < M; ++m) if (masks[m])
        for (int t = 0; t <= hs[m]->L; ++t) if (!masks[m][t]) return g.refuse(FNN_ERR_ARG, g.at("masks: null entry for layer " + std::to_string(t), m));
    for (int m = 0; m < M; ++m) {
        if (!hs[m]->table16) return g.refuse(FNN_ERR_STATE, g.at("ipnn_set_table has not been called", m));
        if (hs[m]->duo_failed) return g.refuse(FNN_ERR_STATE, g.at("an earlier step failed (StripDuo swap timed out): re-create the handle", m));
    }
    ipnn_handle* h0 = g.h0;
    std::vector<IpDraw> draws((size_t)M);
    if (seeds) for (int m = 0; m < M; ++m) draws[m] = IpDraw{seeds[m], steps[m]};
    auto mask_of = [&](int m) { return masks ? masks[m] : nullptr; };
    auto draw_of = [&](int m) { return seeds ? &draws[m] : nullptr; };
    auto logits_of = [&](int m) { return logits_out ? logits_out[m] : nullptr; };
    if (M == 1) {                                                     // one model: its solo step, reported as the group reports
        const int rc = ip_train_step(h0, ids, wts, y, B, mask_of(0), draw_of(0), logits_of(0), loss_sum_out);
        return rc == FNN_OK ? rc : g.refuse(rc, g.at(h0->err, 0));
    }
    IRC(g.enter());
    const hipStream_t st = h0->st;
    // the members by path and class
    std::vector<IpStepClass> cls;
    std::vector<int> own;
    for (int m = 0; m < M; ++m) {
        if (!ip_step_shares(hs[m])) { own.push_back(m); continue; }
        const IpStepClass c{ip_pred_class_of(hs[m], wts != nullptr), hs[m]->plan.group.wg0[hs[m]->L + 1], ip_bwd_rows(hs[m]),
                            hs[m]->plan.bwd.capA, hs[m]->plan.bwd.capB};
        cls[class_index(cls, c)].pc.members.push_back(m);
    }
    const int ng = M - (int)own.size();
    if (seeds) for (int m = 0; m < M; ++m)                            // every byte a step reads is drawn by that step
        if (!hs[m]->mask0) IHK(h0, hipMalloc((void**)&hs[m]->mask0, (size_t)hs[m]->Bmax * hs[m]->d[0]));
    if (loss_sum_out && !h0->step_pack) {
        IHK(h0, hipMalloc((void**)&h0->step_pack, (size_t)2 * IPNN_STEP_MAX_MODELS * 4));
        IHK(h0, hipHostMalloc((void**)&h0->step_pack_host, (size_t)2 * IPNN_STEP_MAX_MODELS * 4, hipHostMallocDefault));
    }
    // one array per call: the group members' records class by class, then (with loss_sum_out) a header for every other member
    const size_t elem = h0->step_ring.elem, nrec = (size_t)ng + (loss_sum_out ? own.size() : 0);
    size_t slot = 0;
    const char* d = nullptr;
    std::vector<IpSortClass> sorts;
    std::vector<IpStepExt> ext(cls.size());
    int Ba = 0;
    if (nrec) {
        IHK(h0, ring_take(h0->step_ring, nrec, &slot));
        char* a = h0->step_ring.host_bytes(slot);
        d = h0->step_ring.dev_bytes(slot);
        size_t pos = 0;
        for (size_t i = 0; i < cls.size(); ++i) for (int m : cls[i].pc.members) {
            ipnn_handle* h = hs[m];
            const size_t s = class_index(sorts, IpSortClass{h->n_rows, h->key64, h->kn.sort_merge4, h}, [](const IpSortClass& a, const IpSortClass& b) {
                return a.n_rows == b.n_rows && a.key64 == b.key64 && a.merge4 == b.merge4; });
            const IpCall c = ip_step_call(h, ids, wts, y, B, mask_of(m), draw_of(m), logits_of(m));
            Ba = c.Ba;
            float* pack = loss_sum_out ? h0->step_pack + 2 * m : nullptr;
            if (h->bf16) ip_fill_step_arg<bf16_t>(h, m, c, sorts[s].first->rg.rec, pack, a + pos * elem);
            else ip_fill_step_arg<float>(h, m, c, sorts[s].first->rg.rec, pack, a + pos * elem);
            const IpStepArg<float>* r = reinterpret_cast<const IpStepArg<float>*>(a + pos * elem);      // (the extents sit in front of the typed fields)
            if (r->drawn) ext[i].n_draw = std::max(ext[i].n_draw, r->n_mask); else ext[i].n_maskT = std::max(ext[i].n_maskT, r->n_mask);
            ext[i].n_scat1 = std::max(ext[i].n_scat1, r->n_scat1);
            ++pos;
        }
        if (loss_sum_out) for (int m : own) {
            IpStepArg<float> r{};
            r.model = m; r.pack = h0->step_pack + 2 * m; r.u.err = hs[m]->err_flag; r.u.loss_sum = hs[m]->loss_dev;
            memcpy(a + pos * elem, &r, sizeof(r));
            ++pos;
        }
        IHK(h0, ring_send(h0->step_ring, slot, nrec, st));
    }
    for (const IpSortClass& s : sorts) {                              // the batch's ids, grouped once per grouping class
        const IpCall c = ip_step_call(s.first, ids, wts, y, B, nullptr, nullptr, nullptr);
        ip_sort_ids(s.first, c, st);                                  // into the class's first member's buffers, as its solo step sorts
    }
    {
        size_t pos = 0;
        for (size_t i = 0; i < cls.size(); ++i) {
            const std::vector<int>& mem = cls[i].pc.members;
            const ipnn_handle* h = hs[mem[0]];
            IHK(h0, cls[i].pc.bf16 ? ip_launch_step_class<bf16_t>(h, cls[i], ext[i], d + pos * elem, Ba, st)
                                   : ip_launch_step_class<float>(h, cls[i], ext[i], d + pos * elem, Ba, st));
            for (int m : mem) if (hs[m]->adam) {                      // an Adam / FTRL member's b and table pass: the solo step's own launches
                ipnn_handle* hm = hs[m];
                const float lr_step = ip_lr_step(hm, hm->adam_t + 1);
                const IpCall c = ip_step_call(hm, ids, wts, y, B, nullptr, nullptr, nullptr);
                ip_b_update(hm, c, st, lr_step);
                ip_adam_table(hm, st, lr_step);
            }
            pos += mem.size();
        }
    }
    IHK(h0, hipGetLastError());
    for (const IpStepClass& c : cls) for (int m : c.pc.members) if (hs[m]->adam) hs[m]->adam_t += 1;      // accepted: the members have made a step
    for (int m : own) {
        ipnn_handle* h = hs[m];
        const int rc = on_stream(h, st, [&] {
            IRC(ip_step_enqueue(h, ids, wts, y, B, mask_of(m), draw_of(m), logits_of(m)));
            return loss_sum_out ? ip_join(h) : FNN_OK;                // (the loss is summed in the update launch: join it)
        });
        if (rc != FNN_OK) return g.member_failed(rc, h, m);
    }
    if (!loss_sum_out) return g.leave();
    if (!own.empty()) {
        hipLaunchKernelGGL(k_ip_step_pack, dim3(1), dim3(256), 0, st, d + (size_t)ng * elem, elem, (int)own.size());
        IHK(h0, hipGetLastError());
    }
    IHK(h0, hipMemcpyAsync(h0->step_pack_host, h0->step_pack, (size_t)2 * M * 4, hipMemcpyDeviceToHost, st));
    const int rj = g.leave();
    IHK(h0, hipStreamSynchronize(st));
    if (rj != FNN_OK) return rj;
    std::string bad, gave_up;
    for (int m = 0; m < M; ++m) {
        loss_sum_out[m] = h0->step_pack_host[2 * m];
        const int f = (int)h0->step_pack_host[2 * m + 1];
        if (f & 2) { hs[m]->duo_failed = true; eval_list_add(gave_up, m); }      // as ipnn_sync judges a solo step
        else if (f & 1) eval_list_add(bad, m);
    }
    if (!gave_up.empty())
        return g.refuse(FNN_ERR_HIP, "a strip workgroup gave up waiting for its partner (StripDuo swap) in model(s) " + gave_up +
                        ": that step's outputs are invalid and its dense update was not applied; those handles refuse further train steps" +
                        (bad.empty() ? "" : "; feature id outside [0, n_rows) of model(s) " + bad));
    if (!bad.empty()) return g.refuse(FNN_ERR_RANGE, "feature id outside [0, n_rows) of model(s) " + bad);
    return FNN_OK;
}

int ipnn_prof_enable(ipnn_handle* h, int on)
{
    if (!h) return FNN_ERR_ARG;
    IRC(ip_join(h));
    IHK(h, hipStreamSynchronize(h->st));
    if (on) { for (auto& kv : h->prof_ev) for (auto& p : kv.second) { hipEventDestroy(p.first); hipEventDestroy(p.second); } h->prof_ev.clear(); }
    h->prof = on != 0;
    return FNN_OK;
}

// IPNN_STAMPS: the last step's per-layer time stamps of the strip launches of one direction ("fwd" / "bwd"), to stderr
static int ip_print_stamps(ipnn_handle* h, const char* which)
{
    const bool fwd = !strcmp(which, "fwd"), tail = h->kn.stamps == 2;
    const bool duo = h->duo_xch != nullptr && !tail;           // pairs: even workgroups run the whole stack, odd ones the wide products only
    const int nwg = tail ? h->ldT / 16 : h->ldT / (h->bf16 ? 32 : 16) * (duo ? 2 : 1), np = h->L + 3, step = duo ? 2 : 1;
    std::vector<long long> st((size_t)nwg * 16);
    IHK(h, hipMemcpy(st.data(), h->stamps + (fwd ? 0 : (size_t)(h->ldT / 16) * 16), st.size() * 8, hipMemcpyDeviceToHost));
    auto at = [&](int w, int i) { return st[(size_t)w * 16 + i]; };
    for (int par = 0; par < step; ++par) {
        long long t0 = at(par, 0), t1 = 0; int cnt = 0;
        for (int w = par; w < nwg; w += step) {
            t0 = std::min(t0, at(w, 0)); ++cnt;
            for (int i = 0; i < np; ++i) t1 = std::max(t1, at(w, i));
        }
        fprintf(stderr, "[ipnn stamps %s%s] %d workgroups, first start -> last stamp %lld ticks; avg ticks per phase (load, then products):", which,
                duo ? (par ? " odd" : " even") : "", cnt, t1 - t0);
        for (int i = 1; i < np; ++i) {
            double s2 = 0; int c2 = 0;
            for (int w = par; w < nwg; w += step) if (at(w, i) > at(w, i - 1)) { s2 += (double)(at(w, i) - at(w, i - 1)); ++c2; }
            fprintf(stderr, " %.0f", c2 ? s2 / c2 : 0.0);
        }
        double sk = 0, d3[3] = {0, 0, 0};
        for (int w = par; w < nwg; w += step) sk += (double)(at(w, 0) - t0);
        fprintf(stderr, " | avg start skew %.0f", sk / cnt);
        if (h->kn.stamp_sel >= 0 && fwd) {
            for (int w = par; w < nwg; w += step) for (int i = 0; i < 3; ++i) d3[i] += (double)(at(w, 11 + i) - at(w, 10 + i));
            fprintf(stderr, " | product %d, wave 0, last block: aux+product %.0f, next+prefetch %.0f, epilogue %.0f", h->kn.stamp_sel, d3[0] / cnt, d3[1] / cnt, d3[2] / cnt);
        } else if (duo) {
            for (int w = par; w < nwg; w += 2) for (int i = 0; i < 3; ++i) d3[i] += (double)at(w, 11 + i);
            fprintf(stderr, " | swaps in all: drain+barrier %.0f, flag wait %.0f, pull %.0f", d3[0] / cnt, d3[1] / cnt, d3[2] / cnt);
        }
        fprintf(stderr, "\n");
    }
    return FNN_OK;
}

int ipnn_prof_get(ipnn_handle* h, const char* which, double* avg_ms)
{
    if (!h || !which || !avg_ms) return FNN_ERR_ARG;
    IRC(ip_join(h));
    IHK(h, hipStreamSynchronize(h->st));
    *avg_ms = 0.0;
    if (h->stamps && (!strcmp(which, "fwd") || !strcmp(which, "bwd"))) IRC(ip_print_stamps(h, which));
    auto it = h->prof_ev.find(which);
    if (it == h->prof_ev.end() || it->second.empty()) return FNN_OK;
    double tot = 0.0;
    for (auto& p : it->second) { float ms = 0.f; if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) tot += ms; }
    *avg_ms = tot / (double)it->second.size();
    return FNN_OK;
}

}  // extern "C"
