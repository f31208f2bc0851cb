// ip_strip_kernels.hip.h -- the deep stack of the inner-product family as strip kernels (gfx950 only): a workgroup, or a pair
// of them (StripDuo), carries a strip of 16 or 32 examples through every product of the stack, forward or backward, the
// activations staying in LDS.  A part of the unit ipnn_api.hip, which alone includes it.  The GEMM epilogues (EpiIpFwd /
// EpiIpOut / EpiIpBwd: also those of the one-launch-per-product form, k_gemm_ft, under IPNN_STRIP=0), then the strip machinery
// (StripFwdArgs / StripBwdArgs, the item walk, the bodies), then the kernels k_ip_strip_fwd, k_ip_strip_bwd and k_ip_strip_tail.
// Launched by ip_strips_fwd / ip_strips_bwd (ipnn_api.hip), which pick the instance through ip_strip_sel / ip_strip_tail_sel;
// strip_fwd_body / strip_bwd_body are also the bodies of the group forms (ip_group_kernels.hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fnn_kernels.hip.h"
#include "ip_gather_kernels.hip.h"

namespace {
using namespace fnn;

// ------------------------------------------------------------------------------------------
// GEMM epilogues of the deep stack.
// ------------------------------------------------------------------------------------------
// All activation / delta matrices of the stack are FRAGMENT-TILED (ft_off) in both orientations:
// xF (rows = examples, k = units) feeds the next forward / backward-data product, xT (rows = units,
// k = examples) the weight-gradient product.  Only dz1 (f32, for the inner-product backward) is row-major.
// The epilogues compute the 4 values a lane owns (rows r0 .. r0+3 of one column); k_gemm_ft writes both
// layouts.  Keep-masks are read TRANSPOSED ([unit][example], k_mask_T in ip_step_kernels.hip.h): a lane's 4 rows are 4
// consecutive bytes, one dword load; activations for act' come from xT the same way (one 8-byte load).
// Transposed keep-masks are tiled like a fragment-tiled operand of bytes: 16 units x 32 examples = one 512-byte
// block, so that a 32-example strip reads whole blocks (and a 128-row GEMM tile four of them per 16 units).
__host__ __device__ inline size_t mask_off(int col, int row, int ldT) {
    return ((size_t)(col >> 4) * (ldT >> 5) + (row >> 5)) * 512 + (col & 15) * 32 + (row & 31);
}
// Every epilogue is split in two: load() fetches what the lane's 4 values need from memory (it can be issued
// before the product's k-loop), apply() turns the accumulator into the values; pre() is both.
template <typename T> struct EpiIpFwd {      // a_t = mask/keep * act(l_t); ones column at d
    static constexpr bool TILE = true;
    T* outF; int ld; T* outT; int ldT; const uint8_t* maskT; float inv_keep; int act, d, B;
    struct Aux { unsigned mb; };
    __device__ Aux load(int r0, int col) const {
        Aux x{0x01010101u};
        if (maskT && col < d) x.mb = *reinterpret_cast<const unsigned*>(maskT + mask_off(col, r0, ldT));
        return x;
    }
    __device__ void pre(int r0, int col, const f32x4& acc, float v[4]) const { apply(load(r0, col), r0, col, acc, v); }
    // the activation is a wave-uniform run-time value: branch on it once per fragment (or once per block, applyA)
    __device__ void apply(const Aux& ax, int r0, int col, const f32x4& acc, float v[4]) const {
        if (act == A_RELU) applyA<A_RELU>(ax, r0, col, acc, v);
        else if (act == A_TANH) applyA<A_TANH>(ax, r0, col, acc, v);
        else applyA<A_SIG>(ax, r0, col, acc, v);
    }
    // PLAIN: every row of the block is an example (< B) and every column a real unit (< d): no edge selects
    template <int ACT, bool PLAIN = false> __device__ void applyA(const Aux& ax, int r0, int col, const f32x4& acc, float v[4]) const {
        const unsigned mb = ax.mb;
        const float sc = maskT ? inv_keep : 1.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float x = ip_act_c<ACT>(acc[r]) * ((float)((mb >> (8 * r)) & 0xffu) * sc);
            if (!PLAIN) {
                x = col < d ? x : (col == d ? 1.0f : 0.f);
                x = (r0 + r < B) ? x : 0.f;
            }
            v[r] = x;
        }
    }
    __device__ bool plain(int row_end, int col_end) const { return row_end <= B && col_end <= d; }
};
template <typename T> struct EpiIpOut {      // logits (column 0), loss, delta = sigmoid(logit) - y
    static constexpr bool TILE = true;
    T* outF; int ld; T* outT; int ldT; const float* y; float* logits; float* loss_t; float* p_out; int B;
    float gscale;            // 1 for a summed loss, 1 / B for tf.reduce_mean (python/FNN_IP_L7.py:83-86): scales every gradient of the step
    struct Aux { };
    __device__ Aux load(int, int) const { return Aux{}; }
    __device__ void pre(int r0, int col, const f32x4& acc, float v[4]) const { apply(Aux{}, r0, col, acc, v); }
    __device__ void apply(const Aux&, int r0, int col, const f32x4& acc, float v[4]) const {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = r0 + r;
            float x = 0.f;
            if (col == 0 && t < B) {
                const float z = acc[r], p = 1.0f / (1.0f + expf(-z));
                if (logits) logits[t] = z;
                if (p_out) p_out[t] = p;
                // (the fused product spelled out: left to the compiler, the solo strip kernels fuse it and the group forms, the same
                // code in another kernel, did not -- one rounding apart for labels other than 0 and 1)
                if (y) { x = (p - y[t]) * gscale; loss_t[t] = fmaf(-z, y[t], fmaxf(z, 0.f)) + log1pf(expf(-fabsf(z))); }
            } else if (col == 0 && loss_t) loss_t[t] = 0.f;
            v[r] = x;
        }
    }
};
template <typename T> struct EpiIpBwd {      // delta l_t = (delta l_{t+1} W^T) * mask/keep * act'(l_t)
    static constexpr bool TILE = true;
    T* outF; int ld; T* outT; int ldT; float* out32; int ld32; const T* aT; const uint8_t* maskT; float inv_keep, keep; int act, d, B;
    const int* ref;          // layer 0 (out32 != null): slot column -> reference column, -1 = padding
    struct Aux { unsigned mb; float4 u; bool real; };
    __device__ Aux load(int r0, int col) const {
        Aux x{0x01010101u, make_float4(0.f, 0.f, 0.f, 0.f), ref ? ref[col] >= 0 : col < d};
        if (x.real) {
            if (maskT) x.mb = *reinterpret_cast<const unsigned*>(maskT + mask_off(col, r0, ldT));
            x.u = load4(aT + ft_off<T>(col, r0, ldT));
        }
        return x;
    }
    __device__ void pre(int r0, int col, const f32x4& acc, float v[4]) const { apply(load(r0, col), r0, col, acc, v); }
    __device__ void apply(const Aux& ax, int r0, int col, const f32x4& acc, float v[4]) const {
        if (act == A_RELU) applyA<A_RELU>(ax, r0, col, acc, v);
        else if (act == A_TANH) applyA<A_TANH>(ax, r0, col, acc, v);
        else applyA<A_SIG>(ax, r0, col, acc, v);
    }
    template <int ACT, bool PLAIN = false> __device__ void applyA(const Aux& ax, int r0, int col, const f32x4& acc, float v[4]) const {
        const unsigned mb = ax.mb;
        const float uu[4] = {ax.u.x, ax.u.y, ax.u.z, ax.u.w};
        const float sc = maskT ? inv_keep : 1.0f, ks = maskT ? keep : 1.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float m = (float)((mb >> (8 * r)) & 0xffu);
            float x = acc[r] * m * sc * ip_dact_u_c<ACT>(uu[r] * ks);                      // act(l_t) where m = 1
            if (!PLAIN) x = (r0 + r < B && ax.real) ? x : 0.f;
            v[r] = x;
            if (out32) out32[(size_t)(r0 + r) * ld32 + col] = x;
        }
    }
    __device__ bool plain(int row_end, int col_end) const { return !ref && !out32 && row_end <= B && col_end <= d; }
};

// ------------------------------------------------------------------------------------------
// Strip kernels: the whole deep stack for a strip of 16 RT examples inside ONE workgroup, forward
// (k_ip_strip_fwd: L + 1 products, activations, loss / output delta) and backward-data
// (k_ip_strip_bwd: L + 1 products down to dz1).  As separate GEMM launches these products are bound by
// fixed costs -- per launch ~4 us of launch, ~1.5 us of pipeline fill, ~5 us of epilogue writing both
// operand layouts and ~5 us of cold operands, against 3-8 us of L2-bound main loop -- 16 times per step.
// Here a strip's activations stay in LDS (two ping-pong tiles in fragment order, so an A fragment is
// one conflict-free ds_read_b128 per lane; each tile as wide as the widest layer that lands in it: capA, capB), each wave owns 64-column blocks of a layer's output and
// streams the weights (fragment-tiled, L2-resident) straight into B fragments, and only what the
// weight-gradient products need goes to HBM: the transposed activations / deltas.  Every workgroup
// reads every weight once per pass: 16 RT FLOP per L2 byte, which is what bounds these kernels.
// ------------------------------------------------------------------------------------------
constexpr int STRIP_MAXP = IPNN_MAX_HIDDEN + 1;                  // products of the stack
// TWO workgroups per strip (h = blockIdx.x & 1; strip = blockIdx.x >> 1): a 32-example strip occupies one CU and at batch 4096
// that is 128 of the chip's 256, each streaming every weight at the ~75 GB/s one CU draws from L2 -- the bound of these kernels.
// The pair splits every WIDE product by output column blocks (block j belongs to workgroup j & 1), so each CU streams half the
// weights, and swaps halves after it: a workgroup pushes its blocks of the new activation tile to `xch` with write-through
// (sc1) 16-byte stores, drains them, raises its flag, polls its partner's and pulls the partner's blocks into its own LDS tile
// with sc1 loads (MI355X_MICROARCH.md, "Valid forms": every store and load of the handed-off bytes sc1, stores drained before
// the flag, one lane polls, the others load behind a workgroup barrier).  Narrow products (fewer than DUO_MIN_BLOCKS column
// blocks) are computed by BOTH workgroups -- their weights are a few hundred KB, a swap costs more -- and workgroup 0 alone
// writes their outputs.  Workgroups b and b + 8 share an XCD, so the even XCDs only ever stream the even blocks' weights and
// the odd XCDs the odd ones: half the weight footprint per L2.  Flags hold launch_epoch * 16 + (swap index + 1): they only
// grow, so nothing is reset between launches; a poll gives up after DUO_SPIN_LIMIT tries and raises `err` (no hang on a bug).
struct StripDuo { int on; unsigned long long* xch; int* flags; int epoch; int* err; size_t xch_wg; int min_blocks; };
constexpr int DUO_MIN_BLOCKS = 5;                                // default of StripDuo::min_blocks (IPNN_DUO_MIN)
constexpr int DUO_SPIN_LIMIT = 1 << 22;
template <typename T> struct StripFwdArgs {
    const T* a0; int n;                                          // a0: F layout [Ba][Dp0]; n = L + 1
    const T* W[STRIP_MAXP]; int Dp[STRIP_MAXP + 1];              // W[t-1] = wf[t-1]: fragment-tiled [Dp_t][Dp_{t-1}]
    EpiIpFwd<T> ef[STRIP_MAXP]; EpiIpOut<T> eo;                  // ef[t-1], t = 1..L; eo: the output unit
    long long* dbg;                                              // IPNN_STAMPS=1 (diagnostics): s_memtime per layer, 16 per workgroup
    int rot;                                                     // rotate the block order per workgroup (IPNN_STRIP_ROT=0: off)
    StripDuo duo;                                                // two workgroups per strip (see StripDuo); duo.on = 0: one
    int sel;                                                     // IPNN_STAMPS: the product whose first block of wave 0 is stamped in detail (slots 10..14)
    // A launch may cover a RANGE of the stack (round 3: the wide products as pairs of 32-example strips, the narrow tail as 16-example
    // strips on every CU).  has_out = 0: the last product of this launch is a hidden layer whose tile leaves for HBM in the F layout
    // (finalF: the next launch's a0), block by block as it is computed -- no swap, no barrier behind it.
    int has_out; T* finalF;
    // 16-example strips (RT = 1) only: products whose weights are copied into LDS behind the two tiles at the start of the launch
    // (element offset there, or -1: streamed from L2 as usual).  The narrow products are chains of a few k-steps, each an L2 round
    // trip long (~600 ticks with four in flight); from LDS a k-step costs what its MFMAs cost
    int wlds[STRIP_MAXP];
    int warm;                                                    // touch every line of these arguments at the start (see strip_warm_args)
};
template <typename T> struct StripBwdArgs {
    const T* dlast; int n;                                       // delta of the output layer, F layout [Ba][64]
    const T* W[STRIP_MAXP]; int Dp[STRIP_MAXP + 1];              // W[t-1] = wb[t-1]: fragment-tiled [Dp_{t-1}][Dp_t]
    EpiIpBwd<T> eb[STRIP_MAXP];                                  // eb[t-1]: product t -> delta l_{t-1}
    long long* dbg;
    int rot;
    StripDuo duo;
    // bottom = 1: product 1 of this launch is the stack's first (its output is dz1, f32, no tile).  bottom = 0: the launch stops inside
    // the stack and product 1's tile leaves for HBM in the F layout (finalF: the next launch's dlast)
    int bottom; T* finalF;
    int wlds[STRIP_MAXP];                                        // as in StripFwdArgs (index = product index t - 1 of this launch)
    int warm;
};
// The kernels read their per-product arguments (ef[l] / eb[t - 1]: a different 64-byte line of the argument segment per product) with
// scalar loads at the top of each product, behind the barrier: a scalar-cache miss on every wave's critical path, once per product.
// One dword of every line at the start of the launch instead -- all misses in flight together, under the strip's own load.
template <int BYTES> __device__ __forceinline__ void strip_warm_args()
{
    typedef const int __attribute__((address_space(4))) karg_int;
    karg_int* p = (karg_int*)__builtin_amdgcn_kernarg_segment_ptr();
    int s = 0;
#pragma unroll
    for (int o = 0; o < BYTES; o += 64) s |= p[o / 4];
    asm volatile("" :: "s"(s));
}

// one 64-column block of one product: acc[m][n] = sum_k in[16 m ..][k] W[64 blk + 16 n ..][k].
// Weights: five register stages (four k-steps in flight while one multiplies: with two waves per SIMD that
// covers an L2 round trip at the rate the texture path delivers fragments); loads past the end are clamped
// to the last k-step, so the loop has no branch.  The strip's own fragments come from LDS.
// An ITEM of a product is NF of its 16-column fragments: NF = 4 (a 64-column block) everywhere but in the 16-example strips of
// the narrow tail, whose kernels may take finer items (k_ip_strip_*<T, 1, NF>): a 64- or 128-wide product then occupies 4 / 8
// waves instead of 1 / 2, and an item's epilogue is NF / 4 of a block's.  `blk` below is the item index: fragments blk NF + n.
template <typename T, int NF = 4> struct StripB { typename Traits<T>::frag s[4][NF]; };     // k-steps 0..3 of an item's weights, in flight

template <typename T, int NF = 4>
__device__ __forceinline__ void strip_prefetch(StripB<T, NF>& pb, const T* __restrict__ W, const int nkt, const int blk, const int lane)
{
    typedef typename Traits<T>::frag frag;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int n = 0; n < NF; ++n) pb.s[j][n] = *reinterpret_cast<const frag*>(ft_frag<T>(W, blk * NF + n, min(j, nkt - 1), nkt, lane));
}

template <typename T, int RT, int NF = 4>
__device__ __forceinline__ void strip_product(f32x4 (&acc)[RT][NF], StripB<T, NF>& pb, const T* in, const T* __restrict__ W, const int nkt,
                                              const int blk, const int lane)
{
    typedef typename Traits<T>::frag frag;
#pragma unroll
    for (int m = 0; m < RT; ++m)
#pragma unroll
        for (int n = 0; n < NF; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    frag b4[NF];
    frag (&b0)[NF] = pb.s[0]; frag (&b1)[NF] = pb.s[1]; frag (&b2)[NF] = pb.s[2]; frag (&b3)[NF] = pb.s[3];
    const int last = nkt - 1;
    auto loadb = [&](frag* b, const int kt) {
        const int k = min(kt, last);
#pragma unroll
        for (int n = 0; n < NF; ++n) b[n] = *reinterpret_cast<const frag*>(ft_frag<T>(W, blk * NF + n, k, nkt, lane));
    };
    auto mul = [&](const int kt, const frag* b) {
        frag a[RT];
#pragma unroll
        for (int m = 0; m < RT; ++m) a[m] = *reinterpret_cast<const frag*>(ft_frag<T>(in, m, kt, nkt, lane));
#pragma unroll
        for (int m = 0; m < RT; ++m)
#pragma unroll
            for (int n = 0; n < NF; ++n) mma(acc[m][n], a[m], b[n]);
    };
    int kt = 0;
    for (; kt + 5 <= nkt; kt += 5) {
        loadb(b4, kt + 4); mul(kt, b0);
        if (kt + 5 < nkt) loadb(b0, kt + 5);
        mul(kt + 1, b1);
        if (kt + 6 < nkt) loadb(b1, kt + 6);
        mul(kt + 2, b2);
        if (kt + 7 < nkt) loadb(b2, kt + 7);
        mul(kt + 3, b3);
        if (kt + 8 < nkt) loadb(b3, kt + 8);
        mul(kt + 4, b4);
    }
    if (kt < nkt) mul(kt, b0);
    if (kt + 1 < nkt) mul(kt + 1, b1);
    if (kt + 2 < nkt) mul(kt + 2, b2);
    if (kt + 3 < nkt) mul(kt + 3, b3);
}

// what the epilogue of a block reads from memory (keep-mask bytes, activations for act'), fetched before the k-loop
template <typename T, int RT, int NF, typename Epi>
__device__ __forceinline__ void strip_aux(typename Epi::Aux (&ax)[RT][NF], const Epi& epi, const int row0, const int blk, const int lane)
{
    const int rq = 4 * (lane >> 4), cl = lane & 15;
#pragma unroll
    for (int m = 0; m < RT; ++m)
#pragma unroll
        for (int n = 0; n < NF; ++n) ax[m][n] = epi.load(row0 + m * 16 + rq, (blk * NF + n) * 16 + cl);
}

// epilogue of a block: the lane's values through `epi.apply`, the transposed layout to HBM (8-byte pieces),
// the strip's own layout to the LDS tile `out` (the next product's A operand) when there is a next product
template <int ACT, bool PLAIN, typename T, int RT, int NF, typename Epi>
__device__ __forceinline__ void strip_epilogue_a(f32x4 (&acc)[RT][NF], const typename Epi::Aux (&ax)[RT][NF], const Epi& epi, T* out, const int N,
                                                 const int row0, const int blk, const int lane)
{
    const int rq = 4 * (lane >> 4), cl = lane & 15, col0 = blk * NF * 16;
    T* const outT = epi.outT ? epi.outT + ft_off<T>(col0 + cl, row0 + rq, epi.ldT) : nullptr;   // + n * 16 units, + m * 16 examples
    // (the item's first column is a multiple of 16 NF: with NF < 4 offsets of n * 16 columns still add without a carry into the k-step)
    T* const outL = out ? out + ft_off<T>(rq, col0 + cl, N) : nullptr;
    const size_t tn = ft_off<T>(16, 0, epi.ldT), tm = ft_off<T>(0, 16, epi.ldT);    // strides: 16 units, 16 examples (ldT % KS == 0)
#pragma unroll
    for (int m = 0; m < RT; ++m)
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            float v[4];
            const int col = col0 + n * 16 + cl;
            epi.template applyA<ACT, PLAIN>(ax[m][n], row0 + m * 16 + rq, col, acc[m][n], v);
            if (outT) store4(outT + n * tn + m * tm, v[0], v[1], v[2], v[3]);
            if (outL) {
                T* o = outL + ft_off<T>(m * 16, n * 16, N);       // (row tile m, column offset 16 n): additive in this layout
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r * Traits<T>::EPL] = (T)v[r];
            }
        }
}
template <typename T, int RT, int NF, typename Epi>
__device__ __forceinline__ void strip_epilogue(f32x4 (&acc)[RT][NF], const typename Epi::Aux (&ax)[RT][NF], const Epi& epi, T* out, const int N,
                                               const int row0, const int blk, const int lane)
{   // one branch on the activation and on "interior block" per block
    const bool pl = epi.plain(row0 + RT * 16, (blk + 1) * NF * 16);
#define STRIP_EPI(ACT) do { if (pl) strip_epilogue_a<ACT, true, T, RT, NF, Epi>(acc, ax, epi, out, N, row0, blk, lane); \
                            else strip_epilogue_a<ACT, false, T, RT, NF, Epi>(acc, ax, epi, out, N, row0, blk, lane); } while (0)
    if (epi.act == A_RELU) STRIP_EPI(A_RELU);
    else if (epi.act == A_TANH) STRIP_EPI(A_TANH);
    else STRIP_EPI(A_SIG);
#undef STRIP_EPI
}

template <typename T> __device__ __forceinline__ void strip_load(T* dst, const T* __restrict__ src, const int nfrag16)
{   // nfrag16 16-byte pieces, contiguous in both
    typedef typename Traits<T>::frag frag;
    const int nt = blockDim.x;
    for (int i0 = threadIdx.x; i0 < nfrag16; i0 += nt * 4) {     // four loads in flight per thread before the first LDS store
        frag v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = i0 + nt * k; if (i < nfrag16) v[k] = reinterpret_cast<const frag*>(src)[i]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = i0 + nt * k; if (i < nfrag16) reinterpret_cast<frag*>(dst)[i] = v[k]; }
    }
}

#define STRIP_STAMP(i) do { if (a.dbg && threadIdx.x == 0) a.dbg[(size_t)blockIdx.x * 16 + (i)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
constexpr int STRIP_NW = 8;                                      // waves per strip workgroup (2 per SIMD: 256 registers each)
// A wave's blocks of the stack in order: (product p, list index w), (p, w + NW), ... then the next product it has a
// block in.  The weights of the NEXT block are requested before the current block's epilogue (they do not
// depend on the strip), so the barrier between two products and the epilogue hide their L2 round trip.
// A workgroup's LIST of a product's column blocks: all nblk of them, or -- a wide product of a pair (StripDuo) -- the
// (nblk - h + 1) / 2 blocks j with j & 1 == h.
struct StripItem { int p, blk; };
__device__ __forceinline__ bool duo_split(const StripDuo& d, const int nblk) { return d.on && nblk >= d.min_blocks; }
__device__ __forceinline__ int duo_count(const bool split, const int nblk, const int h) { return split ? (nblk - h + 1) >> 1 : nblk; }
// Workgroups walk their list in rotated order (list entry i of a workgroup with rotation g is entry (i + g) mod cnt), so
// that the workgroups of an XCD do not all stream the same weights -- the same L2 channels -- at the same moment.
// (per items per 64-column block: entry r of the list is sub-item r % per of the workgroup's own block r / per)
__device__ __forceinline__ int strip_phys(const bool split, const int i, const int cnt, const int h, const int rot, const int per = 1) {
    const int r = (i + rot) % cnt, ob = r / per;
    return (split ? 2 * ob + h : ob) * per + r % per;
}
template <typename T> __device__ __forceinline__ bool strip_has_out(const StripFwdArgs<T>& a) { return a.has_out != 0; }
template <typename T> __device__ __forceinline__ bool strip_has_out(const StripBwdArgs<T>&) { return false; }
// items of a product in a workgroup's list: `per` items per 64-column block (4 / NF; pairs split whole blocks: per = 1 there);
// the output unit is ONE item whatever its padded width (column 0 is the only unit)
template <typename A> __device__ __forceinline__ int strip_items(const A& a, const int p, const bool fwd, const int h, const int per)
{
    const int nblk = fwd ? a.Dp[p + 1] / 64 : a.Dp[a.n - p - 1] / 64;
    if (fwd && strip_has_out(a) && p == a.n - 1) return 1;
    return duo_count(duo_split(a.duo, nblk), nblk, h) * per;
}
template <typename A> __device__ __forceinline__ StripItem strip_next(const A& a, StripItem it, const int wave, const bool fwd, const int h, const int per,
                                                                     const int nw = STRIP_NW)
{   // fwd: product p has Dp[p + 1] / 64 blocks (the output unit, p = n - 1: one); bwd: product index q = n - t, Dp[t - 1] / 64 blocks
    it.blk += nw;
    for (;;) {
        if (it.p >= a.n) return it;
        if (it.blk < strip_items(a, it.p, fwd, h, per)) return it;
        it.p += 1; it.blk = wave;
    }
}

// ---- the swap of a pair (StripDuo).  xch of workgroup (strip, h): [2 parities][own block r = j >> 1][RT][256] 8-byte words,
// a block's RT x 2 KB in the order they have in the LDS tile (row tile m: k-steps 2 j and 2 j + 1 are adjacent there).
typedef unsigned int duo_u32x4 __attribute__((ext_vector_type(4)));
// 16-byte write-through stores / L1-bypassing loads of the swap buffer (raw buffer instructions with the sc1 cache policy: the
// compiler keeps their wait counts, unlike inline assembly; 8-byte accesses run at 0.54-0.70 of the 16-byte rate)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t duo_rsrc(const StripDuo& d) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)d.xch, 0, (int)(d.xch_wg * 8 * (size_t)gridDim.x), 0x00020000);
}
template <typename T, int RT, int NF = 4>
__device__ __forceinline__ void duo_push(const StripDuo& d, const T* out, const int N, const int item, const int parity, const int lane)
{   // by the wave that has just written item `item` (NF fragments of block j = item NF / 4) of the tile `out` (LDS operations of one
    // wave complete in order); a block's RT x 2 KB keep the order they have in the LDS tile, so an item's 16-byte pieces are a run of it
    constexpr int PER = 4 / NF, PIECES = 16 * NF * (int)sizeof(T);       // 16-byte pieces per row tile: 128 (a block), 64, 32
    const int j = item / PER, sub = item % PER;
    const __amdgpu_buffer_rsrc_t rs = duo_rsrc(d);
    const size_t dst = ((size_t)blockIdx.x * d.xch_wg + (size_t)parity * (d.xch_wg >> 1) + (size_t)(j >> 1) * (RT * 256)) * 8 + (size_t)sub * PIECES * 16;     // bytes
#pragma unroll
    for (int m = 0; m < RT; ++m) {
        const duo_u32x4* src = reinterpret_cast<const duo_u32x4*>(out + ft_off<T>(m * 16, item * NF * 16, N));
        if (PIECES >= 128) {
            const duo_u32x4 v0 = src[lane], v1 = src[lane + 64];
            __builtin_amdgcn_raw_buffer_store_b128(v0, rs, (int)(dst + m * 2048 + lane * 16), 0, 16);                // aux 16 = sc1: write-through
            __builtin_amdgcn_raw_buffer_store_b128(v1, rs, (int)(dst + m * 2048 + (lane + 64) * 16), 0, 16);
        } else if (lane < PIECES) {
            const duo_u32x4 v0 = src[lane];
            __builtin_amdgcn_raw_buffer_store_b128(v0, rs, (int)(dst + m * 2048 + lane * 16), 0, 16);
        }
    }
}
// block j of the tile `out`, just written by this wave, to its place in an F-layout operand in HBM (plain 16-byte stores; the
// strip's row tiles are contiguous there, so the tile's own offsets apply): the hand-over between two launches of a split stack
template <typename T, int RT, int NF = 4>
__device__ __forceinline__ void strip_final_push(T* __restrict__ dstF, const T* out, const int N, const int sidx, const int j, const int lane)
{   // item j = columns 16 NF j ..: per row tile 16 x 16 NF elements, contiguous in the fragment-tiled layout (NF = 1, bf16: half a fragment)
    constexpr int PIECES = 16 * NF * (int)sizeof(T);             // 16-byte pieces per row tile
    T* base = dstF + (size_t)sidx * RT * 16 * N;
#pragma unroll
    for (int m = 0; m < RT; ++m) {
        const size_t o = ft_off<T>(m * 16, j * NF * 16, N);
        const duo_u32x4* src = reinterpret_cast<const duo_u32x4*>(out + o);
        duo_u32x4* dst = reinterpret_cast<duo_u32x4*>(base + o);
        if (PIECES >= 128) {
            duo_u32x4 v[PIECES / 64 > 0 ? PIECES / 64 : 1];
#pragma unroll
            for (int i = 0; i < PIECES / 64; ++i) v[i] = src[lane + 64 * i];
#pragma unroll
            for (int i = 0; i < PIECES / 64; ++i) dst[lane + 64 * i] = v[i];
        } else if (lane < PIECES) dst[lane] = src[lane];
    }
}
// every wave has drained its pushes -> flag -> the partner's flag -> the partner's blocks into `out`.  `pull` = false: this
// workgroup has nothing left to compute (it only publishes).  All 64 NW threads call it.
template <typename T, int RT, int NW = STRIP_NW>
__device__ __forceinline__ void duo_swap(const StripDuo& d, T* out, const int N, const int nblk, const int h, const int parity, const int seq,
                                         const bool pull, long long* dbg)
{
    long long ta = 0, tb = 0;
    if (dbg && threadIdx.x == 0) ta = (long long)__builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this wave's sc1 stores have left (and whatever else it had in flight)
    lds_barrier();
    const int want = d.epoch * 16 + seq;
    if (dbg && threadIdx.x == 0) { tb = (long long)__builtin_amdgcn_s_memtime(); dbg[11] += tb - ta; }    // drain + barrier
    if (threadIdx.x == 0) {
        __hip_atomic_store(d.flags + blockIdx.x, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (pull) {
            int n = 0;
            while (__hip_atomic_load(d.flags + (blockIdx.x ^ 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
                __builtin_amdgcn_s_sleep(2);
                if (++n > DUO_SPIN_LIMIT) { atomicOr(d.err, 2); break; }      // a partner that never arrives: report, do not hang
            }
        }
    }
    if (!pull) return;
    lds_barrier();
    if (dbg && threadIdx.x == 0) { ta = (long long)__builtin_amdgcn_s_memtime(); dbg[12] += ta - tb; }    // flag + the partner's
    // a block = RT x 2 KB = RT x 128 pieces of 16 bytes: threads 0..255 take the partner's blocks 0, 2, ..., threads 256..511 the odd ones
    const int ph = h ^ 1, cntp = (nblk - ph + 1) >> 1, t = threadIdx.x, pc = t & 255, m = pc >> 7, idx = pc & 127;
    constexpr int G = NW / 4;                                        // groups of 256 threads: group g takes the partner's blocks g, g + G, ...
    const __amdgpu_buffer_rsrc_t rs = duo_rsrc(d);
    const size_t src = ((size_t)(blockIdx.x ^ 1) * d.xch_wg + (size_t)parity * (d.xch_wg >> 1)) * 8 + (size_t)pc * 16;                 // bytes
    for (int r0 = 0; r0 < cntp && m < RT; r0 += 4 * G) {             // four loads in flight per thread
        duo_u32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = r0 + (t >> 8) + G * k;
            if (r < cntp) v[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(src + (size_t)r * (RT * 2048)), 0, 16);           // sc1: from L2
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = r0 + (t >> 8) + G * k;
            if (r < cntp) reinterpret_cast<duo_u32x4*>(out + ft_off<T>(m * 16, (2 * r + ph) * 64, N))[idx] = v[k];
        }
    }
    if (dbg && threadIdx.x == 0) dbg[13] += (long long)__builtin_amdgcn_s_memtime() - ta;                  // pull (thread 0's share)
}

extern __shared__ __align__(16) unsigned char strip_smem[];   // the strip kernels' dynamic LDS: tiles [RT * 16][capA] and [RT * 16][capB] (+ LDS weight copies)
template <typename T, int RT, int NF, int NW>
__device__ __forceinline__ void strip_fwd_body(const StripFwdArgs<T>& a, const int capA, const int capB)
{
    constexpr int EPL = Traits<T>::EPL, KS = Traits<T>::KS, PER = 4 / NF;       // NF < 4: no pairs (the host launches those without StripDuo)
    T* in = reinterpret_cast<T*>(strip_smem);                    // tile A: the layers at even positions of the launch's range
    T* out = in + (size_t)RT * 16 * capA;                        // tile B: the odd ones
    T* wl = out + (size_t)RT * 16 * capB;                        // RT = 1: LDS copies of the small products' weights (a.wlds)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = a.duo.on ? (int)(blockIdx.x & 1) : 0, sidx = a.duo.on ? (int)(blockIdx.x >> 1) : (int)blockIdx.x;
    const int row0 = sidx * RT * 16;
    STRIP_STAMP(0);
    if (a.warm) strip_warm_args<(int)sizeof(StripFwdArgs<T>)>();
    if (a.dbg && threadIdx.x == 0) { for (int i = 10; i < 16; ++i) a.dbg[(size_t)blockIdx.x * 16 + i] = 0; }
    StripB<T, NF> pb;
    StripItem nx = strip_next(a, StripItem{0, wave - NW}, wave, true, h, PER, NW);
    const int rot = (a.rot == 1) ? (sidx >> 3) : (a.rot == 2 ? sidx : 0);   // workgroups g, g + 8, ... share an XCD
    // the last product this workgroup computes: the second of a pair stops behind the last product the pair splits
    int last = a.n - 1;
    if (h == 1) { last = -1; for (int p = 0; p < a.n; ++p) if (duo_split(a.duo, a.Dp[p + 1] / 64)) last = p; }
    auto blocks = [&](const int p, bool& split, int& cnt) { split = duo_split(a.duo, a.Dp[p + 1] / 64); cnt = strip_items(a, p, true, h, PER); };
    auto prefetch_next = [&]() {
        if (nx.p < a.n && nx.p <= last) {
            bool sp; int cn; blocks(nx.p, sp, cn);
            const int wo = RT == 1 ? a.wlds[nx.p] : -1;
            // (spelled from the LDS array itself: through the captured pointer the address space was lost and the loads came out flat_)
            if (wo >= 0) strip_prefetch<T, NF>(pb, reinterpret_cast<const T*>(strip_smem) + (size_t)RT * 16 * (capA + capB) + wo, a.Dp[nx.p] / KS, strip_phys(sp, nx.blk, cn, h, rot, PER), lane);
            else strip_prefetch<T, NF>(pb, a.W[nx.p], a.Dp[nx.p] / KS, strip_phys(sp, nx.blk, cn, h, rot, PER), lane);
        }
    };
    if (RT == 1) {                                               // the small products' weights -> LDS (contiguous, fragment-tiled: offsets carry over)
        const bool first_lds = nx.p < a.n && a.wlds[nx.p] >= 0;
        if (!first_lds) prefetch_next();                         // a first item streamed from L2 (the big first product) does not wait for the copy
        bool any = false;
        for (int p = 0; p < a.n; ++p)
            if (a.wlds[p] >= 0) { strip_load<T>(wl + a.wlds[p], a.W[p], a.Dp[p] * a.Dp[p + 1] / EPL); any = true; }
        if (any) lds_barrier();                                  // (uniform: `any` comes from the arguments)
        if (first_lds) prefetch_next();
    } else prefetch_next();
    // the strip of a0: row tiles RT sidx .. of an F-layout operand are contiguous
    strip_load<T>(in, a.a0 + (size_t)sidx * RT * 16 * a.Dp[0], RT * 16 * a.Dp[0] / EPL);
    lds_barrier();
    STRIP_STAMP(1);
    f32x4 acc[RT][NF];
    int seq = 0;
    for (int l = 0; l <= last; ++l) {
        const int nkt = a.Dp[l] / KS, N = a.Dp[l + 1];
        const bool hidden = !a.has_out || l + 1 < a.n;
        const bool fin = !a.has_out && l + 1 == a.n;            // the launch stops here: blocks go to HBM, nobody swaps
        bool split; int cnt; blocks(l, split, cnt);
        while (nx.p == l) {
            const int blk = strip_phys(split, nx.blk, cnt, h, rot, PER);
            const bool det = a.dbg && l == a.sel && threadIdx.x == 0;
#define DET(i) do { if (det) a.dbg[(size_t)blockIdx.x * 16 + (i)] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
            DET(10);
            if (hidden) {
                EpiIpFwd<T> ef = a.ef[l];                       // the layer's epilogue parameters: scalar registers, loaded once
                if (a.duo.on && !split && h == 1) ef.outT = nullptr;     // (not reached: the second workgroup computes split products only)
                typename EpiIpFwd<T>::Aux ax[RT][NF];
                strip_aux<T, RT, NF>(ax, ef, row0, blk, lane);
                if (RT == 1 && a.wlds[l] >= 0) strip_product<T, RT, NF>(acc, pb, in, wl + a.wlds[l], nkt, blk, lane);
                else strip_product<T, RT, NF>(acc, pb, in, a.W[l], nkt, blk, lane);
                DET(11);
                nx = strip_next(a, nx, wave, true, h, PER, NW);
                prefetch_next();
                DET(12);
                strip_epilogue<T, RT, NF>(acc, ax, ef, out, N, row0, blk, lane);
                DET(13);
                if (fin) { if (split || h == 0) strip_final_push<T, RT, NF>(a.finalF, out, N, sidx, blk, lane); }
                else if (split) duo_push<T, RT, NF>(a.duo, out, N, blk, seq & 1, lane);
            } else {                                              // the output unit: logits, loss, delta (column 0): item 0 = fragment 0 ..
                if (RT == 1 && a.wlds[l] >= 0) strip_product<T, RT, NF>(acc, pb, in, wl + a.wlds[l], nkt, blk, lane);
                else strip_product<T, RT, NF>(acc, pb, in, a.W[l], nkt, blk, lane);
                nx.p = a.n;
                const EpiIpOut<T> eo = a.eo;
                const int rq = 4 * (lane >> 4), cl = lane & 15;
                // only column 0 is a unit: columns 1..63 of the delta (both layouts) are zero and stay zero -- the
                // buffers are zero-filled at creation and these kernels are their only writers -- so one fragment per row tile
#pragma unroll
                for (int m = 0; m < RT; ++m) {
                    float v[4];
                    const int r0 = row0 + m * 16 + rq;
                    eo.pre(r0, cl, acc[m][0], v);
                    if (eo.outT) store4(eo.outT + ft_off<T>(cl, r0, eo.ldT), v[0], v[1], v[2], v[3]);
                    if (eo.outF) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) eo.outF[ft_off<T>(r0 + r, cl, eo.ld)] = (T)v[r];
                    }
                }
            }
        }
        if (split && !fin) { duo_swap<T, RT, NW>(a.duo, out, N, N / 64, h, seq & 1, seq + 1, l < last, a.dbg ? a.dbg + (size_t)blockIdx.x * 16 : nullptr); ++seq; }
        if (hidden && !fin) lds_barrier();
        STRIP_STAMP(2 + l);
        T* t = in; in = out; out = t;
    }
}
template <typename T, int RT, int NF = 4, int NW = STRIP_NW>
static __global__ __launch_bounds__(64 * NW) void k_ip_strip_fwd(const StripFwdArgs<T> a, const int capA, const int capB) { strip_fwd_body<T, RT, NF, NW>(a, capA, capB); }

template <typename T, int RT, int NF, int NW>
__device__ __forceinline__ void strip_bwd_body(const StripBwdArgs<T>& a, const int capA, const int capB)
{
    constexpr int EPL = Traits<T>::EPL, KS = Traits<T>::KS, PER = 4 / NF;
    T* in = reinterpret_cast<T*>(strip_smem);                    // tile A: delta l_n, delta l_{n-2}, ...
    T* out = in + (size_t)RT * 16 * capA;                        // tile B: delta l_{n-1}, ...
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = a.duo.on ? (int)(blockIdx.x & 1) : 0, sidx = a.duo.on ? (int)(blockIdx.x >> 1) : (int)blockIdx.x;
    const int row0 = sidx * RT * 16;
    STRIP_STAMP(0);
    if (a.warm) strip_warm_args<(int)sizeof(StripBwdArgs<T>)>();
    if (a.dbg && threadIdx.x == 0) { for (int i = 10; i < 16; ++i) a.dbg[(size_t)blockIdx.x * 16 + i] = 0; }
    T* wl = out + (size_t)RT * 16 * capB;                        // RT = 1: LDS copies of the small products' weights (a.wlds)
    StripB<T, NF> pb;                                             // item index q = n - t: product t = n - q
    StripItem nx = strip_next(a, StripItem{0, wave - NW}, wave, false, h, PER, NW);
    const int rot = (a.rot == 1) ? (sidx >> 3) : (a.rot == 2 ? sidx : 0);   // workgroups g, g + 8, ... share an XCD
    auto blocks = [&](const int q, bool& split, int& cnt) { split = duo_split(a.duo, a.Dp[a.n - q - 1] / 64); cnt = strip_items(a, q, false, h, PER); };
    auto prefetch_next = [&]() {
        if (nx.p < a.n) {
            bool sp; int cn; blocks(nx.p, sp, cn);
            const int wo = RT == 1 ? a.wlds[a.n - nx.p - 1] : -1;
            if (wo >= 0) strip_prefetch<T, NF>(pb, reinterpret_cast<const T*>(strip_smem) + (size_t)RT * 16 * (capA + capB) + wo, a.Dp[a.n - nx.p] / KS, strip_phys(sp, nx.blk, cn, h, rot, PER), lane);
            else strip_prefetch<T, NF>(pb, a.W[a.n - nx.p - 1], a.Dp[a.n - nx.p] / KS, strip_phys(sp, nx.blk, cn, h, rot, PER), lane);
        }
    };
    if (RT == 1) {                                               // the small products' weights -> LDS; in the backward launch they are the FIRST products
        bool any = false;
        for (int p = 0; p < a.n; ++p)
            if (a.wlds[p] >= 0) { strip_load<T>(wl + a.wlds[p], a.W[p], a.Dp[p] * a.Dp[p + 1] / EPL); any = true; }
        if (any) lds_barrier();                                  // the first item's prefetch reads them
    }
    prefetch_next();
    strip_load<T>(in, a.dlast + (size_t)sidx * RT * 16 * a.Dp[a.n], RT * 16 * a.Dp[a.n] / EPL);
    lds_barrier();
    STRIP_STAMP(1);
    f32x4 acc[RT][NF];
    int seq = 0;
    for (int t = a.n; t >= 1; --t) {                              // delta l_{t-1} = (delta l_t . W_t^T) * mask * act'
        const int nkt = a.Dp[t] / KS, N = a.Dp[t - 1], q = a.n - t;
        bool split; int cnt; blocks(q, split, cnt);
        while (nx.p == q) {
            const int blk = strip_phys(split, nx.blk, cnt, h, rot, PER);
            EpiIpBwd<T> eb = a.eb[t - 1];
            if (a.duo.on && !split && h == 1) { eb.outT = nullptr; eb.out32 = nullptr; }   // a narrow product of a pair: both compute it, the first one stores it
            typename EpiIpBwd<T>::Aux ax[RT][NF];
            strip_aux<T, RT, NF>(ax, eb, row0, blk, lane);
            if (RT == 1 && a.wlds[t - 1] >= 0) strip_product<T, RT, NF>(acc, pb, in, wl + a.wlds[t - 1], nkt, blk, lane);
            else strip_product<T, RT, NF>(acc, pb, in, a.W[t - 1], nkt, blk, lane);
            nx = strip_next(a, nx, wave, false, h, PER, NW);
            prefetch_next();
            strip_epilogue<T, RT, NF>(acc, ax, eb, (t > 1 || !a.bottom) ? out : nullptr, N, row0, blk, lane);
            if (split && t > 1) duo_push<T, RT, NF>(a.duo, out, N, blk, seq & 1, lane);
            if (t == 1 && !a.bottom && (split || h == 0)) strip_final_push<T, RT, NF>(a.finalF, out, N, sidx, blk, lane);
        }
        if (split && t > 1) { duo_swap<T, RT, NW>(a.duo, out, N, N / 64, h, seq & 1, seq + 1, true, a.dbg ? a.dbg + (size_t)blockIdx.x * 16 : nullptr); ++seq; }
        if (t > 1) lds_barrier();
        STRIP_STAMP(2 + q);
        T* x = in; in = out; out = x;
    }
}
template <typename T, int RT, int NF = 4, int NW = STRIP_NW>
static __global__ __launch_bounds__(64 * NW) void k_ip_strip_bwd(const StripBwdArgs<T> a, const int capA, const int capB) { strip_bwd_body<T, RT, NF, NW>(a, capA, capB); }
// The narrow tail of a training step, forward then backward, in ONE launch of 16-example strips: what the backward half reads of the
// forward half -- the output delta (F layout, 16 x 64) and the transposed activations its act' needs -- was stored by this same
// workgroup, so a drained store queue and a workgroup barrier order them (this CU's L1 holds none of those lines: the forward half
// never read them; stores write through to the L2).  Saves a launch and the second tile load's cold start.
template <typename T, int NF, int NW>
static __global__ __launch_bounds__(64 * NW) void k_ip_strip_tail(const StripFwdArgs<T> fa, const StripBwdArgs<T> ba, const int capA, const int capB)
{
    strip_fwd_body<T, 1, NF, NW>(fa, capA, capB);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    strip_bwd_body<T, 1, NF, NW>(ba, capA, capB);
}

}  // namespace
