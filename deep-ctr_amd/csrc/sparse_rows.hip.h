// sparse_rows.hip.h -- the sparse-row update that every model family shares: the grouping of the (row, t) keys and the
// two-level segmented update that follows (gfx950 only).  Keys, then grouping, then update, then the host side.
//
// A6  sparse-row SGD with the reference's sequential duplicate semantics
// (python/FNN_wnzh.py:299-306): a row hit by m examples (in example order) with slot gradients
// g_1..g_m ends at  row*c^m - lr * sum_j g_j * c^(m-j),  c = 1 - 2*lambda_fm*lr/b_size.
//   k_sort    per field: bitonic sort of the (row, t) keys -- in registers for strides inside a
//             thread, with wave shuffles inside a wave, through LDS only for the few strides that
//             cross waves -- then every sorted entry learns its segment [s, e) by binary search
//             -> rec {row, t, s, e}.  Independent of the gradients: runs on a side stream under
//             the MLP.
//   k_scat1   a chunk of 16 consecutive sorted entries is folded per slot of the row: g * c^(e-1-pos)
//             added in f64 per run of equal rows, in entry order.  A thread owns one 16-byte
//             quarter-column of the chunk (scat1q_body: only the quarters with live slots, 3 of 4
//             at K = 11) and has a sub-batch of 8 entries' gradients, old rows and decay factors
//             in flight at once; scat1h_body, the default, gives each sub-batch a thread of its
//             own, so that both are in flight at once; FNN_SCAT1_FORM=slot runs the earliest form,
//             a 16-lane group per chunk with a lane per slot (scat1_body); all three give the same
//             bits.  The weight
//             is absolute inside the segment, so partial sums of a segment cut by chunk borders
//             simply add up.  Runs that lie inside the chunk are written back at once; the
//             others leave a partial and the run that opens a multi-chunk segment registers its
//             owner.
//   k_scat2   one wave per registered owner (scat2w_body; FNN_SCAT2_FORM=block: one workgroup,
//             scat2_body -- the same bits) adds the partials of its segment in a fixed
//             order and writes the row.  No float atomics anywhere: the result is bitwise
//             reproducible.
#pragma once
#include "fnn_kernels.hip.h"

namespace fnn {

// ------------------------------------------------------------------------------------------
// Grouping role: a field's 4096 (row, t) keys sorted in two independent phases -- 16 runs of 256
// keys, each bitonic-sorted inside ONE wave's registers, and (SortArgs::merge4) a workgroup's four runs
// merged into one of 1024 (phase A), then a merge by rank in which every key finds its final place
// and its segment [s, e) with binary searches over the 16 or 4 runs (phase B).  32-bit keys
// (row << 12 | t) when n_rows * 4096 fits, else 64-bit.  Measured against
// the single-kernel bitonic network it replaced: 34 us -> 2 x ~4 us of role time.
// ------------------------------------------------------------------------------------------
template <typename KT> struct KeyTraits;
template <> struct KeyTraits<unsigned> { static constexpr int SH = 12; };
template <> struct KeyTraits<unsigned long long> { static constexpr int SH = 32; };

struct SortArgs {
    const int32_t* ids; int B, F; int64_t n_rows; int4* rec; int* owner_cnt; int nblk; void* skeys;
    // bag mode only (null otherwise): which rows of this batch sit in MORE THAN ONE column.  The grouping is per column, and a
    // row's update is one read-modify-write per column segment -- two columns holding the same row (python/SNN_RBM.py:248-253
    // lists a line's active features in line order, so a feature's column depends on the line) would race.  Every segment head
    // claims its row with atomicMax(tag_first[row], stamp << 6 | column); a head that finds this batch's stamp already there
    // under another column marks tag_shared[row] = stamp, and the update launches (at least one kernel boundary later) add
    // into such rows with float atomics instead (scatw1_body / scatw2_body).  Stamps grow with every grouping: no reset pass.
    int* tag_first; int* tag_shared; int stamp;
    int merge4;      // 1: phase A leaves 4 runs of 1024 keys per field and phase B merges those (FNN_SORT_RUNS=4, the default); 0: 16 runs of 256
};

constexpr int SORT_N = 4096;     // keys per field handled by the union-kernel path (B <= 4096)

template <typename KT> __host__ __device__ constexpr size_t sort_lds_bytes() { return (size_t)SORT_N * sizeof(KT); }
// dynamic LDS of phase A (sortA_body): a workgroup's four wave runs, merged in place into one run of 1024 keys; none for the 16-run form
template <typename KT> inline size_t sortA_lds_bytes(const int merge4) { return merge4 ? (size_t)1024 * sizeof(KT) : 0; }
// FNN_SORT_RUNS=16|4, read where a handle is created: the runs per field that phase A leaves for the rank merge.  `dflt` (1: four
// runs) is the handle's own choice: four where phase A rides beside longer roles (the FNN step on FM rows: 35.6 -> 33.6 us per
// step) and in the inner-product step (level), sixteen where the longer phase A is a launch of its own in front of the merge
// (FM pre-training: 29.3 -> 30.8 us with four) and in bag mode (the SNN step: 47.5 -> 48.1) -- profiles/step_stores16_sort4_ab.json
inline int sort_merge4_env(const int dflt)
{
    const char* e = getenv("FNN_SORT_RUNS");
    const int v = e ? atoi(e) : 0;
    return v == 16 ? 0 : (v == 4 ? 1 : dflt);
}

// Invalid entries (t >= B, id outside the table) carry the all-ones row, so that every key of a
// field is distinct (the rank merges below need a strict total order) and they sort to the end.
template <typename KT> __device__ __forceinline__ KT inv_row() { return (~(KT)0) >> KeyTraits<KT>::SH; }

// first index in the ascending run q[0 .. 1 << LOG) whose key is >= v (branch-free; q in LDS)
template <typename KT, int LOG>
__device__ __forceinline__ int lower_bound_pow2(const KT* q, const KT v) {
    int base = 0;
#pragma unroll
    for (int s = 1 << (LOG - 1); s >= 1; s >>= 1) base += (q[base + s - 1] < v) ? s : 0;
    return base + ((q[base] < v) ? 1 : 0);
}

// Phase A of the split sort: every wave bitonic-sorts a run of 256 keys in registers (4 per lane:
// strides below 4 inside the lane, the rest wave shuffles -- no LDS, no barriers) and stores it.
// One workgroup = 4 runs = a quarter of a field; so.nblk = 4 F.
// so.merge4: the workgroup then merges its four wave runs by rank into ONE run of 1024 keys (LDS, one barrier: a key's place is
// its index in its own run plus the keys below it in the three others, 27 reads each) -- the rank merge of phase B, the longest
// role of its launch, then searches 4 runs of 1024 instead of 16 of 256: 11 searches per key instead of 48.
// M4 = so.merge4 as a template parameter: the union launches are instantiated per form (see sortB_form).
template <typename KT, bool M4>
__device__ __forceinline__ void sortA_form(const SortArgs& so, const int blk, unsigned char* smem)
{
    constexpr int SH = KeyTraits<KT>::SH;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, F = so.F, B = so.B;
    const int f = blk >> 2, base = (blk & 3) * 1024 + wave * 256;
    KT key[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {                             // initial order inside a run is free
        const int t = base + a * 64 + lane;
        KT row = inv_row<KT>();
        if (t < B) {
            const int64_t id = so.ids[(size_t)t * F + f];
            if (id >= 0 && id < so.n_rows) row = (KT)id;
        }
        key[a] = (row << SH) | (KT)t;
    }
    const int i0 = lane * 4;                                  // position of key[0] in the run
#pragma unroll
    for (int k = 2; k <= 256; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j < 4) {
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const int b = a ^ j;
                    if (b > a) {
                        const bool up = ((i0 + a) & k) == 0;
                        const KT x = key[a], y = key[b];
                        const KT mn = x < y ? x : y, mx = x < y ? y : x;
                        key[a] = up ? mn : mx; key[b] = up ? mx : mn;
                    }
                }
            } else {
                const bool keepmin = ((i0 & j) == 0) == ((i0 & k) == 0);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const KT other = __shfl_xor(key[a], j >> 2);
                    const KT mine = key[a];
                    const KT mn = mine < other ? mine : other, mx = mine < other ? other : mine;
                    key[a] = keepmin ? mn : mx;
                }
            }
        }
    }
    if constexpr (M4) {
        KT* s_run = reinterpret_cast<KT*>(smem);              // [4][256] the workgroup's wave runs
#pragma unroll
        for (int a = 0; a < 4; ++a) s_run[wave * 256 + i0 + a] = key[a];
        __syncthreads();
        int place[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) place[a] = i0 + a;
        // 12 searches (3 other runs x 4 keys) in lockstep: every step issues 12 independent LDS reads.  Keys are distinct, so
        // "keys below" is the same strict order from both sides of a pair of runs.
        int bq[3][4];
#pragma unroll
        for (int o = 0; o < 3; ++o)
#pragma unroll
            for (int a = 0; a < 4; ++a) bq[o][a] = ((wave + 1 + o) & 3) * 256;
#pragma unroll
        for (int st = 128; st >= 1; st >>= 1)
#pragma unroll
            for (int o = 0; o < 3; ++o)
#pragma unroll
                for (int a = 0; a < 4; ++a) bq[o][a] += s_run[bq[o][a] + st - 1] < key[a] ? st : 0;
#pragma unroll
        for (int o = 0; o < 3; ++o)
#pragma unroll
            for (int a = 0; a < 4; ++a)
                place[a] += bq[o][a] - ((wave + 1 + o) & 3) * 256 + (s_run[bq[o][a]] < key[a] ? 1 : 0);
        KT* out = static_cast<KT*>(so.skeys) + (size_t)f * SORT_N + (blk & 3) * 1024;
#pragma unroll
        for (int a = 0; a < 4; ++a) out[place[a]] = key[a];
        return;
    }
    KT* out = static_cast<KT*>(so.skeys) + (size_t)f * SORT_N + base + i0;
#pragma unroll
    for (int a = 0; a < 4; ++a) out[a] = key[a];
}
template <typename KT>
__device__ __forceinline__ void sortA_body(const SortArgs& so, const int blk, unsigned char* smem)
{
    if (so.merge4) sortA_form<KT, true>(so, blk, smem); else sortA_form<KT, false>(so, blk, smem);
}

// Phase B of the split sort: merge by RANK.  A key's place in the field's final order is its index
// in its own run plus, for each of the 15 other runs, the number of keys below it (a 9-step binary
// search in LDS); its segment [s, e) comes the same way: s = keys below (row, 0), e = keys below
// (row + 1, 0).  Every key is independent -- one thread per key, 16 workgroups per field
// (so.nblk = 16 F), one barrier -- instead of a 15 us chain of dependent merge stages.
// M4: the runs are 4 of 1024 keys (so.merge4); a template parameter, because launch 3 carrying both forms behind a run-time
// branch took 107 VGPRs against the 16-run form's 94 (gfx950, hipcc 7.2) -- the union launches are instantiated per form, so
// that a handle on sixteen runs launches the code it launched before there were two.
template <typename KT, bool M4>
__device__ __forceinline__ void sortB_form(const SortArgs& so, const int blk, unsigned char* smem)
{
    constexpr int SH = KeyTraits<KT>::SH;
    KT* s_key = reinterpret_cast<KT*>(smem);                 // [4096] the 16 sorted runs
    const int tid = threadIdx.x, f = blk >> 4, run = blk & 15;
    if (blk == 0 && tid == 0) *so.owner_cnt = 0;
    const KT* in = static_cast<const KT*>(so.skeys) + (size_t)f * SORT_N;
#pragma unroll
    for (int a = 0; a < 16; ++a) s_key[a * 256 + tid] = in[a * 256 + tid];
    __syncthreads();
    const KT key = s_key[run * 256 + tid];
    const KT row = key >> SH, lo_key = row << SH, hi_key = (row + 1) << SH;    // row + 1 wraps only for invalid entries
    int pos = 0, s = 0, e = 0;
    if constexpr (M4) {
        // 4 runs of 1024 keys: the key's index in its own run plus its rank in the 3 others, and the ranks of lo_key / hi_key in
        // all 4 -- 11 searches of 10 steps in lockstep (about 120 LDS reads against the 16-run form's 480)
        const int own = run >> 2;
        int bp[3], bs[4], be[4];
#pragma unroll
        for (int o = 0; o < 3; ++o) bp[o] = ((own + 1 + o) & 3) * 1024;
#pragma unroll
        for (int r = 0; r < 4; ++r) bs[r] = be[r] = r * 1024;
#pragma unroll
        for (int st = 512; st >= 1; st >>= 1) {
#pragma unroll
            for (int o = 0; o < 3; ++o) bp[o] += s_key[bp[o] + st - 1] < key ? st : 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const KT vs = s_key[bs[r] + st - 1], ve = s_key[be[r] + st - 1];
                bs[r] += vs < lo_key ? st : 0; be[r] += ve < hi_key ? st : 0;
            }
        }
        pos = (run & 3) * 256 + tid;
#pragma unroll
        for (int o = 0; o < 3; ++o) pos += bp[o] - ((own + 1 + o) & 3) * 1024 + (s_key[bp[o]] < key ? 1 : 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s += bs[r] - r * 1024 + (s_key[bs[r]] < lo_key ? 1 : 0);
            e += be[r] - r * 1024 + (s_key[be[r]] < hi_key ? 1 : 0);
        }
    } else {
        // 48 binary searches (16 runs x {key, lo_key, hi_key}) advance in lockstep, so that every step
        // issues 48 independent LDS reads instead of one dependent read at a time.  The search of the
        // key in its own run returns its own index, so no run is special.
        int bp[16], bs[16], be[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) bp[r] = bs[r] = be[r] = r * 256;
#pragma unroll
        for (int st = 128; st >= 1; st >>= 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const KT vp = s_key[bp[r] + st - 1], vs = s_key[bs[r] + st - 1], ve = s_key[be[r] + st - 1];
                bp[r] += vp < key ? st : 0; bs[r] += vs < lo_key ? st : 0; be[r] += ve < hi_key ? st : 0;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            pos += bp[r] - r * 256 + (s_key[bp[r]] < key ? 1 : 0);
            s += bs[r] - r * 256 + (s_key[bs[r]] < lo_key ? 1 : 0);
            e += be[r] - r * 256 + (s_key[be[r]] < hi_key ? 1 : 0);
        }
    }
    int4 rr = make_int4(-1, 0, 0, 0);
    if (row != inv_row<KT>()) {
        rr = make_int4((int)row, (int)(key & (((KT)1 << SH) - 1)), s, e);
        if (so.tag_first && pos == s) {                            // head of its segment: one claim per (row, column)
            const int mine = (so.stamp << 6) | f;
            const int old = atomicMax(&so.tag_first[(size_t)row], mine);
            if ((old >> 6) == so.stamp && old != mine) so.tag_shared[(size_t)row] = so.stamp;
        }
    }
    so.rec[(size_t)f * SORT_N + pos] = rr;
}
template <typename KT>
__device__ __forceinline__ void sortB_body(const SortArgs& so, const int blk, unsigned char* smem)
{
    if (so.merge4) sortB_form<KT, true>(so, blk, smem); else sortB_form<KT, false>(so, blk, smem);
}

// The split sort as two plain launches, for a batch nobody announced (fnn_prefetch_ids) and for
// the inner-product family: 4 F then 16 F workgroups, ~7 us each instead of the 34 us single-kernel
// bitonic network.
template <typename KT>
static __global__ __launch_bounds__(256) void k_sortA(const SortArgs so)
{
    extern __shared__ __align__(16) unsigned char smem[];
    sortA_body<KT>(so, blockIdx.x, smem);
}
template <typename KT>
static __global__ __launch_bounds__(256) void k_sortB(const SortArgs so)
{
    extern __shared__ __align__(16) unsigned char smem[];
    sortB_body<KT>(so, blockIdx.x, smem);
}

// `extra` [n_extra][3] = (example t, field, row): features of a line that a LATER feature of the same field shadowed in the
// gather (python/FNN_wnzh.py:91-96 keeps the last) but that the reference's update loop still visits (:300-306 walks every
// feature of the line).  They join their field's keys as (row, t) pairs behind the B regular ones, so that a row's decay
// powers and gradient terms count every visit in example order; N2 >= B + (extras of any one field).
template <int KPT>
static __global__ __launch_bounds__(1024) void k_sort(const int32_t* __restrict__ ids, int B, int F,
                                               int64_t n_rows, int N2, int4* __restrict__ rec,
                                               int* __restrict__ owner_cnt, const int32_t* __restrict__ extra, int n_extra,
                                               int* __restrict__ err)
{
    extern __shared__ unsigned long long s_key[];
    __shared__ int s_cnt;
    const int f = blockIdx.x, tid = threadIdx.x;       // blockDim.x == N2 / KPT
    if (f == 0 && tid == 0) *owner_cnt = 0;
    int cnt = 0;
    if (n_extra > 0) {                                 // wave-uniform: the common case pays one compare
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        for (int j = tid; j < n_extra; j += blockDim.x) {
            const int t = extra[3 * j], ff = extra[3 * j + 1]; const int64_t r = extra[3 * j + 2];
            if (ff < 0 || ff >= F || t < 0 || t >= B || r < 0 || r >= n_rows) { if (f == 0) atomicOr(err, 1); continue; }
            if (ff != f) continue;
            const int p = atomicAdd(&s_cnt, 1);
            if (B + p < N2) s_key[B + p] = ((unsigned long long)r << 32) | (unsigned)t;
        }
        __syncthreads();
        cnt = min(s_cnt, N2 - B);
    }
    unsigned long long key[KPT];
#pragma unroll
    for (int a = 0; a < KPT; ++a) {
        const int i = tid * KPT + a;
        unsigned long long kk = ~0ull;
        if (i < B) {
            const int64_t id = ids[(size_t)i * F + f];
            if (id >= 0 && id < n_rows) kk = ((unsigned long long)id << 32) | (unsigned)i;
        } else if (i < B + cnt) kk = s_key[i];
        key[a] = kk;
    }
    if (n_extra > 0) __syncthreads();                  // s_key is reused by the exchange stages
    for (int k = 2; k <= N2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j < KPT) {                              // both elements live in this thread
#pragma unroll
                for (int jj = KPT >> 1; jj > 0; jj >>= 1) {
                    if (j == jj) {
#pragma unroll
                        for (int a = 0; a < KPT; ++a) {
                            const int b = a ^ jj;
                            if (b > a) {
                                const bool up = ((tid * KPT + a) & k) == 0;
                                const unsigned long long x = key[a], y = key[b];
                                if ((x > y) == up) { key[a] = y; key[b] = x; }
                            }
                        }
                    }
                }
            } else if (j < 64 * KPT) {                  // partner lane of the same wave
                const int d = j / KPT;
#pragma unroll
                for (int a = 0; a < KPT; ++a) {
                    const int i = tid * KPT + a;
                    const unsigned long long other = __shfl_xor(key[a], d);
                    const bool keepmin = ((i & j) == 0) == ((i & k) == 0);
                    const unsigned long long mine = key[a];
                    key[a] = keepmin ? (mine < other ? mine : other) : (mine > other ? mine : other);
                }
            } else {                                    // partner in another wave: through LDS
                __syncthreads();
#pragma unroll
                for (int a = 0; a < KPT; ++a) s_key[tid * KPT + a] = key[a];
                __syncthreads();
#pragma unroll
                for (int a = 0; a < KPT; ++a) {
                    const int i = tid * KPT + a;
                    const unsigned long long other = s_key[i ^ j];
                    const bool keepmin = ((i & j) == 0) == ((i & k) == 0);
                    const unsigned long long mine = key[a];
                    key[a] = keepmin ? (mine < other ? mine : other) : (mine > other ? mine : other);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < KPT; ++a) s_key[tid * KPT + a] = key[a];
    __syncthreads();
#pragma unroll
    for (int a = 0; a < KPT; ++a) {
        const int pos = tid * KPT + a;
        const unsigned long long kk = key[a];
        int4 r = make_int4(-1, 0, 0, 0);
        if (kk != ~0ull) {
            const unsigned long long lo_key = kk & 0xffffffff00000000ull;
            const unsigned long long hi_key = lo_key + 0x100000000ull;
            int lo = 0, hi = pos;                     // first index with key >= lo_key
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_key[mid] < lo_key) lo = mid + 1; else hi = mid; }
            const int s = lo;
            lo = pos + 1; hi = N2;                    // first index with key >= hi_key
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_key[mid] < hi_key) lo = mid + 1; else hi = mid; }
            r = make_int4((int)(kk >> 32), (int)(kk & 0xffffffffu), s, lo);
        }
        rec[(size_t)f * N2 + pos] = r;
    }
}

struct ScatArgs {
    const int4* rec; int N2, F, K; const float* gxp; int K1p; const double* cpow; double lr;
    float* table16; double* part; int* owner_cnt; int4* owners;
    int rw;          // 16: FM rows (decayed update); otherwise the bag-table row width (plain sum)
    const int* tag_shared; int stamp;     // bag mode: tag_shared[row] == stamp <=> the row sits in several columns of this batch (SortArgs)
    int gxf;         // wide update (scatw*): floats between two fields' gradients of an example (wide FM rows: rw); 0: one per example (bag)
    int form;        // level 1 of the 16-float rows: SCAT1_QUARTER (scat1q_body), SCAT1_SLOT (scat1_body) or SCAT1_HALF (scat1h_body); set by scat1_blocks
    int form2;       // level 2 of the 16-float rows: SCAT2_BLOCK (scat2_body; what an initialiser that does not name it gets) or SCAT2_WAVE (scat2w_body)
};
enum { SCAT1_QUARTER = 0, SCAT1_SLOT = 1, SCAT1_HALF = 2 };   // a thread per quarter-column of a chunk / a lane per slot / a thread per quarter-column of half a chunk
// bag rows held by several columns of a batch: every column adds its sum with float atomics (a row touched by one column
// only -- the rule on iPinYou lines -- keeps the plain read-modify-write, one rounding)
__device__ __forceinline__ void atomic_add4(float* p, float a, float b, float c, float d) {
    atomicAdd(p, a); atomicAdd(p + 1, b); atomicAdd(p + 2, c); atomicAdd(p + 3, d);
}
__device__ __forceinline__ void scat1_body(const ScatArgs& sa, const int blk)
{
    const int4* __restrict__ rec = sa.rec; const int N2 = sa.N2, F = sa.F, K = sa.K, K1p = sa.K1p;
    const float* __restrict__ gxp = sa.gxp; const double* __restrict__ cpow = sa.cpow; const double lr = sa.lr;
    float* __restrict__ table16 = sa.table16; double* __restrict__ part = sa.part;
    int* __restrict__ owner_cnt = sa.owner_cnt; int4* __restrict__ owners = sa.owners;
    const int l = threadIdx.x & 15;                       // slot of the row
    const int G = (blk * 256 + threadIdx.x) >> 4;         // chunk of 16 sorted entries
    const int NQ = N2 >> 4;
    if (G >= F * NQ) return;
    const int f = G / NQ, q = G % NQ, base = q * 16;
    const int4 mine = rec[(size_t)f * N2 + base + l];
    // both decay factors of an entry depend on its record only: its own weight c^(e-1-pos) and its
    // segment's c^(e-s) -- fetched together with the gradients and the old rows, not after them.
    // (The conditional loads below compile to a branch and a wait per entry: 18 dependent round trips per chunk.  Making all
    // 34 dword loads unconditional was measured SLOWER inside the launch, 16.4 -> 18.2 us.  What did shorten the chain is
    // scat1q_body below -- four times fewer, four times wider loads, 8 entries in flight: the role alone 14.5 -> 12.8 us on the
    // events' clock, launch 2 14.35 -> 13.7 us at split-K 4 and 13.1 us with the eight K slices it then has room for.  This form
    // stays as FNN_SCAT1_FORM=slot.)
    const double wmine = (mine.x >= 0) ? cpow[mine.w - 1 - (base + l)] : 0.0;
    const double cmine = (mine.x >= 0) ? cpow[mine.w - mine.z] : 0.0;
    int row[16], sg[16], eg[16];
    float g[16], wold[16];
    double w[16], cs[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        row[j] = __shfl(mine.x, j, 16);
        const int t = __shfl(mine.y, j, 16);
        sg[j] = __shfl(mine.z, j, 16);
        eg[j] = __shfl(mine.w, j, 16);
        w[j] = __shfl(wmine, j, 16);
        cs[j] = __shfl(cmine, j, 16);
        const bool live = row[j] >= 0 && l < K;
        g[j] = live ? gxp[(size_t)t * K1p + f * SLOT + l] : 0.f;
        wold[j] = live ? table16[(size_t)row[j] * SLOT + l] : 0.f;
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (row[j] < 0) continue;
        acc += (double)g[j] * w[j];
        const bool last = (j == 15) || (row[j + 1 < 16 ? j + 1 : 15] != row[j]);
        if (!last) continue;
        const int s = sg[j], e = eg[j];
        if (s >= base && e <= base + 16) {                 // the whole segment lies in this chunk
            if (l < K) table16[(size_t)row[j] * SLOT + l] = (float)((double)wold[j] * cs[j] - lr * acc);
        } else {
            const int which = (s < base) ? 0 : 1;          // 0: enters from the left; 1: opens here
            part[(((size_t)f * NQ + q) * 2 + which) * SLOT + l] = acc;
            if (which == 1 && l == 0) owners[atomicAdd(owner_cnt, 1)] = make_int4(f, s, e, row[j]);
        }
        acc = 0.0;
    }
}

// The quarter-column form of scat1_body (the narrow-row sibling of scatdw1_body below): a thread owns one 16-byte quarter of a
// chunk of 16 sorted entries, only the (K + 3) / 4 quarters that hold live slots get a thread.  Two sub-batches of 8 entries;
// the records of the second are requested before the data of the first, and a sub-batch's gradients (one float4 per entry), old
// rows and both decay factors go out together: rec -> {gx', rows, cpow} -> stores, twice, instead of a wait per entry.
// Chunks, partials and owners are those of scat1_body (scat2_body reads either), and every slot folds its entries in the same
// order with the same f64 operations, so the two forms give the same bits (tests/test_gpu_scat1_forms.py).
// Needs gxp and table16 16-byte aligned and K1p % 4 == 0 (scat1_blocks checks).
__device__ __forceinline__ void scat1q_body(const ScatArgs& sa, const int blk)
{
    const int N2 = sa.N2, NQ = N2 >> 4, nq = (sa.K + 3) >> 2;
    const int gid = blk * 256 + (int)threadIdx.x;
    const int chunk = gid / nq, q = gid % nq;
    if (chunk >= sa.F * NQ) return;
    const int f = chunk / NQ, qc = chunk % NQ, base = qc * 16;
    const int lim = sa.K - 4 * q;                           // live lanes of this quarter: < 4 only in the last one of a padded row
    const double* __restrict__ cpow = sa.cpow; const double lr = sa.lr;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    int4 rn[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) rn[j] = sa.rec[(size_t)f * N2 + base + j];
    for (int sb = 0; sb < 16; sb += 8) {
        int4 r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = rn[j];
        if (r[0].x < 0) break;                               // invalid keys sort to the end
        if (sb == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) rn[j] = sa.rec[(size_t)f * N2 + base + 8 + j];
        }
        float4 g[8], wold[8];
        double wd[8], cs[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int pos = base + sb + j;
            const bool live = r[j].x >= 0;
            // (dead entries and entries that write no row read example 0 / row 0 / cpow[0]: in bounds, and they stay in cache)
            g[j] = *reinterpret_cast<const float4*>(sa.gxp + (size_t)(live ? r[j].y : 0) * sa.K1p + f * SLOT + 4 * q);
            // the old row and the segment's decay c^(e-s) only where the row is written: the last entry of a segment inside the chunk
            const bool need = live && pos + 1 == r[j].w && r[j].z >= base;
            wold[j] = *reinterpret_cast<const float4*>(sa.table16 + (size_t)(need ? r[j].x : 0) * SLOT + 4 * q);
            wd[j] = cpow[live ? r[j].w - 1 - pos : 0];
            cs[j] = cpow[need ? r[j].w - r[j].z : 0];
        }
        if (lim < 4) {                                       // pad lanes take no gradient
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (lim < 2) g[j].y = 0.f;
                if (lim < 3) g[j].z = 0.f;
                g[j].w = 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (r[j].x < 0) continue;
            a0 += (double)g[j].x * wd[j]; a1 += (double)g[j].y * wd[j]; a2 += (double)g[j].z * wd[j]; a3 += (double)g[j].w * wd[j];
            const int pos = base + sb + j, s = r[j].z, e = r[j].w;
            if (pos + 1 != e && pos + 1 != base + 16) continue;        // the run goes on inside this chunk
            if (s >= base && e <= base + 16) {                       // the whole segment lies in this chunk
                float4 o = make_float4((float)((double)wold[j].x * cs[j] - lr * a0), (float)((double)wold[j].y * cs[j] - lr * a1),
                                       (float)((double)wold[j].z * cs[j] - lr * a2), (float)((double)wold[j].w * cs[j] - lr * a3));
                if (lim < 4) {                                       // pad lanes of the row keep what they hold (scat1_body never writes them)
                    if (lim < 2) o.y = wold[j].y;
                    if (lim < 3) o.z = wold[j].z;
                    o.w = wold[j].w;
                }
                *reinterpret_cast<float4*>(sa.table16 + (size_t)r[j].x * SLOT + 4 * q) = o;
            } else {
                const int which = (s < base) ? 0 : 1;                // 0: enters from the left; 1: opens here
                double* pp = sa.part + (((size_t)f * NQ + qc) * 2 + which) * SLOT + 4 * q;
                pp[0] = a0; pp[1] = a1; pp[2] = a2; pp[3] = a3;
                if (which == 1 && q == 0) sa.owners[atomicAdd(sa.owner_cnt, 1)] = make_int4(f, s, e, r[j].x);
            }
            a0 = a1 = a2 = a3 = 0;
        }
    }
}

// An odd lane takes its even neighbour's value (DPP quad_perm [0, 0, 2, 2]: registers only, no LDS); even lanes keep their own.
__device__ __forceinline__ double lane_below(const double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0xA0, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0xA0, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// The half-chunk form of scat1q_body: a thread owns one 16-byte quarter-column of ONE of the chunk's two sub-batches of 8 entries
// (half = gid & 1: the two halves of a quarter-column sit on adjacent lanes of a wave and leave or stay together).  Both halves'
// gradients, old rows and decay factors are therefore requested at once, and no load waits behind a store to the table:
// rec -> {gx', rows, cpow} -> stores, once.  The f64 fold stays sequential over the chunk: every thread first folds its own eight
// entries to find what its half leaves open at its end (the accumulator restarts where a segment ends), the upper half takes the
// lower half's open sums -- four doubles -- from the lane below as its starting value, and then every thread folds again with
// the stores.  Same expressions in the same entry order as scat1q_body, so the same bits (tests/test_gpu_scat1_half.py);
// chunks, partials, `which` and owners follow the chunk's base as there.  The hand-off sits where both lanes of a pair always
// arrive: a dead upper half is not left early, its entries load example 0 / row 0 like any dead entry.
// Needs what scat1q_body needs (scat1_blocks checks).
// SHARED (FM / LR pre-training with fm_set_shared_rows, fm_api.hip): a row may sit under several columns of the batch, each a
// segment of its own.  The row's mark tag_shared[row] (SortArgs) is requested beside its old value -- the same round trip, row 0
// for entries that write nothing -- and a marked row takes -lr * sum as float atomics, one add per (column, segment), instead of
// the rounded store; FM's update has no per-row decay (cpow == 1), which is what makes the adds legal.  Unmarked rows run the
// expression and the store of SHARED = false, which is the body as it was.
template <bool SHARED>
__device__ __forceinline__ void scat1h_form(const ScatArgs& sa, const int blk)
{
    const int N2 = sa.N2, NQ = N2 >> 4, nq = (sa.K + 3) >> 2;
    const int gid = blk * 256 + (int)threadIdx.x;
    const int half = gid & 1, cq = gid >> 1;
    const int chunk = cq / nq, q = cq % nq;
    if (chunk >= sa.F * NQ) return;                         // both lanes of a pair
    const int f = chunk / NQ, qc = chunk % NQ, base = qc * 16, hb = base + 8 * half;
    const int lim = sa.K - 4 * q;                           // live lanes of this quarter: < 4 only in the last one of a padded row
    const double* __restrict__ cpow = sa.cpow; const double lr = sa.lr;
    int4 r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = sa.rec[(size_t)f * N2 + hb + j];
    float4 g[8], wold[8];
    double wd[8], cs[8];
    int mk[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int pos = hb + j;
        const bool live = r[j].x >= 0;
        // (dead entries and entries that write no row read example 0 / row 0 / cpow[0]: in bounds, and they stay in cache)
        g[j] = *reinterpret_cast<const float4*>(sa.gxp + (size_t)(live ? r[j].y : 0) * sa.K1p + f * SLOT + 4 * q);
        const bool need = live && pos + 1 == r[j].w && r[j].z >= base;
        wold[j] = *reinterpret_cast<const float4*>(sa.table16 + (size_t)(need ? r[j].x : 0) * SLOT + 4 * q);
        wd[j] = cpow[live ? r[j].w - 1 - pos : 0];
        cs[j] = cpow[need ? r[j].w - r[j].z : 0];
        if (SHARED) mk[j] = sa.tag_shared[need ? r[j].x : 0];
    }
    if (lim < 4) {                                           // pad lanes take no gradient
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (lim < 2) g[j].y = 0.f;
            if (lim < 3) g[j].z = 0.f;
            g[j].w = 0.f;
        }
    }
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {                            // what this half leaves open at its end
        if (r[j].x < 0) continue;
        a0 += (double)g[j].x * wd[j]; a1 += (double)g[j].y * wd[j]; a2 += (double)g[j].z * wd[j]; a3 += (double)g[j].w * wd[j];
        if (hb + j + 1 == r[j].w) a0 = a1 = a2 = a3 = 0;
    }
    a0 = lane_below(a0); a1 = lane_below(a1); a2 = lane_below(a2); a3 = lane_below(a3);
    if (!half) a0 = a1 = a2 = a3 = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (r[j].x < 0) continue;
        a0 += (double)g[j].x * wd[j]; a1 += (double)g[j].y * wd[j]; a2 += (double)g[j].z * wd[j]; a3 += (double)g[j].w * wd[j];
        const int pos = hb + j, s = r[j].z, e = r[j].w;
        if (pos + 1 != e && pos + 1 != base + 16) continue;        // the run goes on inside this chunk
        if (SHARED && s >= base && e <= base + 16 && mk[j] == sa.stamp) {   // a marked row: this column's sum is added (pad lanes: +0)
            atomic_add4(sa.table16 + (size_t)r[j].x * SLOT + 4 * q, (float)(-lr * a0), (float)(-lr * a1), (float)(-lr * a2), (float)(-lr * a3));
        } else if (s >= base && e <= base + 16) {                // the whole segment lies in this chunk
            float4 o = make_float4((float)((double)wold[j].x * cs[j] - lr * a0), (float)((double)wold[j].y * cs[j] - lr * a1),
                                   (float)((double)wold[j].z * cs[j] - lr * a2), (float)((double)wold[j].w * cs[j] - lr * a3));
            if (lim < 4) {                                       // pad lanes of the row keep what they hold
                if (lim < 2) o.y = wold[j].y;
                if (lim < 3) o.z = wold[j].z;
                o.w = wold[j].w;
            }
            *reinterpret_cast<float4*>(sa.table16 + (size_t)r[j].x * SLOT + 4 * q) = o;
        } else {
            const int which = (s < base) ? 0 : 1;                // 0: enters from the left; 1: opens here
            double* pp = sa.part + (((size_t)f * NQ + qc) * 2 + which) * SLOT + 4 * q;
            pp[0] = a0; pp[1] = a1; pp[2] = a2; pp[3] = a3;
            if (which == 1 && q == 0) sa.owners[atomicAdd(sa.owner_cnt, 1)] = make_int4(f, s, e, r[j].x);
        }
        a0 = a1 = a2 = a3 = 0;
    }
}
__device__ __forceinline__ void scat1h_body(const ScatArgs& sa, const int blk) { scat1h_form<false>(sa, blk); }

static __global__ __launch_bounds__(256) void k_scat1(const ScatArgs sa)
{
    if (sa.form == SCAT1_SLOT) scat1_body(sa, blockIdx.x);
    else if (sa.form == SCAT1_HALF) scat1h_body(sa, blockIdx.x);
    else scat1q_body(sa, blockIdx.x);
}

// Workgroups of level 1 on 16-float rows -- k_scat1's grid and the scatter role's share of k_step2's -- and the form they run:
// `form` is the handle's choice (FNN_SCAT1_FORM, scat1_form_env), overruled by the slot form where the float4 loads of the
// quarter-column and half-chunk forms would be misaligned.  Every launch site takes its count from here, after the last change to sa.
inline int scat1_blocks(ScatArgs& sa, const int form)
{
    const bool vec_ok = ((uintptr_t)sa.gxp | (uintptr_t)sa.table16) % 16 == 0 && sa.K1p % 4 == 0;
    sa.form = vec_ok ? form : SCAT1_SLOT;
    const size_t nquarters = (size_t)sa.F * (sa.N2 / 16) * ((sa.K + 3) / 4);
    const size_t nthr = sa.form == SCAT1_SLOT ? (size_t)sa.F * sa.N2 : sa.form == SCAT1_HALF ? 2 * nquarters : nquarters;
    return (int)((nthr + 255) / 256);
}
// FNN_SCAT1_FORM=slot|quarter|half, read where a handle is created; unset or unknown: `dflt` -- half, which was measured a gain or
// level for every user of the body (profiles/scat1_half_ab.json)
inline int scat1_form_env(const int dflt = SCAT1_HALF)
{
    const char* e = getenv("FNN_SCAT1_FORM");
    if (!e) return dflt;
    return !strcmp(e, "slot") ? SCAT1_SLOT : !strcmp(e, "quarter") ? SCAT1_QUARTER : !strcmp(e, "half") ? SCAT1_HALF : dflt;
}

__device__ __forceinline__ void scat2_body(const ScatArgs& sa, const int blk, const int nblk, double (*s_sum)[16])
{
    const int4* __restrict__ owners = sa.owners; const int N2 = sa.N2, K = sa.K;
    const double* __restrict__ part = sa.part; const double* __restrict__ cpow = sa.cpow; const double lr = sa.lr;
    float* __restrict__ table16 = sa.table16;
    const int n = *sa.owner_cnt;
    const int l = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const int NQ = N2 >> 4;
    for (int o = blk; o < n; o += nblk) {
        const int4 ow = owners[o];                         // {f, s, e, row}
        const int q0 = ow.y >> 4, q1 = (ow.z - 1) >> 4;
        double sum = 0.0;
        // the row and its decay factor are requested with the partial sums, not after them (one round trip less)
        float* p = table16 + (size_t)ow.w * SLOT + l;
        float wold = 0.f; double cdec = 0.0;
        if (grp == 0 && l < K) { wold = *p; cdec = cpow[ow.z - ow.y]; }
        for (int qb = q0 + grp; qb <= q1; qb += 64) {            // four chunks' partials in flight at a time
            double v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int q = qb + 16 * k;
                v[k] = q <= q1 ? part[(((size_t)ow.x * NQ + q) * 2 + (q == q0 ? 1 : 0)) * SLOT + l] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) sum += v[k];
        }
        s_sum[grp][l] = sum;
        __syncthreads();
        if (grp == 0 && l < K) {
            double tot = 0.0;
#pragma unroll
            for (int gI = 0; gI < 16; ++gI) tot += s_sum[gI][l];
            *p = (float)((double)wold * cdec - lr * tot);
        }
        __syncthreads();
    }
}

// Every lane takes the value lane `src` holds (both halves of the double through the wave's permute: registers only).
__device__ __forceinline__ double lane_from(const double v, const int src)
{
    const int lo = __shfl(__double2loint(v), src, 64), hi = __shfl(__double2hiint(v), src, 64);
    return __hiloint2double(hi, lo);
}

// 64 chunks of a segment, from chunk qb on: lane (j, l) requests slot l of the chunks qb + j + 4 m + 16 k (m, k = 0..3; NK = 1:
// k = 0 only, for a segment of up to 16 chunks) -- all of them before the first is used -- and adds them to its four sums
// S[m] = S_{j + 4 m} in ascending k.  A chunk past the segment's last one reads that last chunk's partial instead (in bounds,
// the same cache line for every such lane) and enters as +0.0, as in scat2_body.
template <int NK>
__device__ __forceinline__ void scat2w_batch(const double* __restrict__ part, const size_t fq, const int q0, const int q1,
                                             const int qb, const int j, const int l, double (&S)[4])
{
    double v[4][NK];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int q = qb + j + 4 * m + 16 * k, qc = min(q, q1);
            const double t = part[((fq + qc) * 2 + (qc == q0 ? 1 : 0)) * SLOT + l];
            v[m][k] = q <= q1 ? t : 0.0;
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int k = 0; k < 4; ++k) S[m] += k < NK ? v[m][k] : 0.0;
    }
}

// The wave form of scat2_body (FNN_SCAT2_FORM=wave): one 64-lane wave per registered owner instead of a 256-thread workgroup,
// no LDS and no workgroup barrier.  A wave's first owner record is requested together with the owner count -- speculatively:
// owners[] holds at least F * N2 / 16 records at every allocation site, and the record is used only once o < n is known --
// and the old row and the segment's decay factor go out with the partial sums: count and record, then the data, then the
// store.  With 256 workgroups the benchmark's ~540 owners all sit in a first iteration; scat2_body walks up to three owners per
// workgroup, each a chain of its own behind two barriers.  Lane (j = lane >> 4, l = lane & 15): l is the row's slot, quarter j
// adds the sums S_g with g = j (mod 4) in scat2_body's order, S_g = (((0 + P_g) + P_{g+16}) + P_{g+32}) + ..., and then every
// lane folds tot = ((0 + S_0) + S_1) + ... + S_15, taking the twelve sums of the other quarters from their lanes: the same f64
// expressions, the same bits (tests/test_gpu_scat2_forms.py).  Control flow is wave-uniform; lanes of quarter 0 with l < K store.
// SHARED: as in scat1h_form -- the owner row's mark goes out with its old value and the partial sums, and a marked row takes
// -lr * tot as one float atomic per live slot.
template <bool SHARED>
__device__ __forceinline__ void scat2w_form(const ScatArgs& sa, const int blk, const int nblk)
{
    const double* __restrict__ part = sa.part; const double* __restrict__ cpow = sa.cpow; const double lr = sa.lr;
    const int lane = threadIdx.x & 63, j = lane >> 4, l = lane & 15;
    const int gw = __builtin_amdgcn_readfirstlane(blk * 4 + ((int)threadIdx.x >> 6));
    const int NQ = sa.N2 >> 4, cap = sa.F * NQ;
    int4 ow = sa.owners[min(gw, cap - 1)];                   // {f, s, e, row}; stale or never written where gw >= n
    const int n = *sa.owner_cnt;
    for (int o = gw; o < n; o += 4 * nblk) {
        if (o != gw) ow = sa.owners[o];
        const int q0 = ow.y >> 4, q1 = (ow.z - 1) >> 4;
        const size_t fq = (size_t)ow.x * NQ;
        float* p = sa.table16 + (size_t)ow.w * SLOT + l;
        const float wold = *p;                               // every lane: all 16 floats of the row exist, no branch around the loads
        const double cdec = cpow[ow.z - ow.y];
        int mk = 0;
        if (SHARED) mk = sa.tag_shared[ow.w];
        double S[4] = {0.0, 0.0, 0.0, 0.0};
        if (q1 - q0 < 16) scat2w_batch<1>(part, fq, q0, q1, q0, j, l, S);
        else for (int qb = q0; qb <= q1; qb += 64) scat2w_batch<4>(part, fq, q0, q1, qb, j, l, S);
        double tot = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) tot += (g & 3) ? lane_from(S[g >> 2], (g & 3) * 16 + l) : S[g >> 2];   // quarter 0 holds S_0, S_4, ...
        if (SHARED && mk == sa.stamp) { if (j == 0 && l < sa.K) atomicAdd(p, (float)(-lr * tot)); }
        else if (j == 0 && l < sa.K) *p = (float)((double)wold * cdec - lr * tot);
    }
}
__device__ __forceinline__ void scat2w_body(const ScatArgs& sa, const int blk, const int nblk) { scat2w_form<false>(sa, blk, nblk); }
enum { SCAT2_BLOCK = 0, SCAT2_WAVE = 1 };                    // ScatArgs::form2: scat2_body / scat2w_body
// FNN_SCAT2_FORM=block|wave, read where a handle is created; unset or unknown: `dflt` -- wave, which was measured a gain or
// level for every user of the body (profiles/scat2_wave_ab.json)
inline int scat2_form_env(const int dflt = SCAT2_WAVE)
{
    const char* e = getenv("FNN_SCAT2_FORM");
    if (!e) return dflt;
    return !strcmp(e, "block") ? SCAT2_BLOCK : !strcmp(e, "wave") ? SCAT2_WAVE : dflt;
}

static __global__ __launch_bounds__(256) void k_scat2(const ScatArgs sa)
{
    __shared__ double s_sum[16][16];
    if (sa.form2 == SCAT2_WAVE) scat2w_body(sa, blockIdx.x, gridDim.x);
    else scat2_body(sa, blockIdx.x, gridDim.x, s_sum);
}

// ------------------------------------------------------------------------------------------
// Sparse-row update of rows rw floats wide: WCH sorted entries per chunk, a thread owns one 16-byte quarter-column of a chunk,
// the gradient of (example t, field f) at gx'[t][f * gxf + l].  Same sorted records as the 16-float rows.  Two updates share
// one body per level:
//   DECAY = false  the bag table (python/SNN_RBM.py:285-291): ww0[f] -= lr * delta_t for every example t that has feature f;
//                  no decay, so a row's result is row - lr * (sum of its deltas) in example order.  The wide FM rows
//                  (k >= 17, fm_api.hip) and the wide inner-product rows take the same update with one gradient row per
//                  (example, field): ScatArgs::gxf.  A row marked tag_shared[row] == stamp takes float atomics (SortArgs).
//   DECAY = true   the decayed update of wide FM rows (FNN_MODE_FM, k >= 17: rows of rw = rup(k, 4) floats): the closed form of
//                  scat1_body / scat2_body -- a row whose segment is [s, e) of the sorted entries ends at row*c^(e-s) - lr *
//                  sum_pos g_pos * c^(e-1-pos).  An entry's weight c^(e-1-pos) is absolute inside its segment, so the level-1
//                  partials of a segment cut by chunk borders simply add up in level 2, which applies c^(e-s) once.  f64 sums,
//                  no float atomics (a row belongs to one field: one group per row), fixed summation order: bit-reproducible.
//                  The pad lanes of a row (l >= K) take no gradient and stay zero.
// ------------------------------------------------------------------------------------------
constexpr int WCH = 32;          // sorted entries per chunk on the wide path (4 sub-batches of 8 loads)

template <bool DECAY>
__device__ __forceinline__ void scatw1_form(const ScatArgs& sa, const int blk)
{
    const int rw = sa.rw, nq = rw >> 2, N2 = sa.N2, NQ = N2 / WCH;
    using gid_t = std::conditional_t<DECAY, int, long>;     // the plain form has always divided a 64-bit thread index: its code stays what it was
    const gid_t gid = (gid_t)blk * 256 + (gid_t)threadIdx.x;
    const int chunk = (int)(gid / nq), q = (int)(gid % nq);
    if (chunk >= sa.F * NQ) return;
    const int f = chunk / NQ, qc = chunk % NQ, base = qc * WCH;
    const int lim = DECAY ? sa.K - 4 * q : 4;               // live lanes of this piece: < 4 only in the last piece of a padded row
    const double* __restrict__ cpow = sa.cpow; const double lr = sa.lr;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    // the records of the NEXT batch of 8 entries are requested together with the gradients / old rows of the current one:
    // one memory round trip per batch instead of two (records, then what they point at)
    int4 rn[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) rn[j] = sa.rec[(size_t)f * N2 + base + j];
    for (int sb = 0; sb < WCH; sb += 8) {
        int4 r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = rn[j];
        if (r[0].x < 0) break;                               // invalid keys sort to the end
        if (sb + 8 < WCH) {
#pragma unroll
            for (int j = 0; j < 8; ++j) rn[j] = sa.rec[(size_t)f * N2 + base + sb + 8 + j];
        }
        float4 g[8], wold[8];
        double wd[8], cs[8];                                 // DECAY only
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int pos = base + sb + j;
            const bool live = r[j].x >= 0;
            g[j] = *reinterpret_cast<const float4*>(sa.gxp + (size_t)(live ? r[j].y : 0) * sa.K1p + (size_t)f * sa.gxf + 4 * q);
            // the old row (and the segment's decay c^(e-s)) only where the row is written: the last entry of a segment inside the chunk
            const bool need = live && pos + 1 == r[j].w && r[j].z >= base;
            // (branch-free: entries that do not need it read row 0, which stays in cache)
            wold[j] = *reinterpret_cast<const float4*>(sa.table16 + (size_t)(need ? r[j].x : 0) * rw + 4 * q);
            if constexpr (DECAY) {
                wd[j] = cpow[live ? r[j].w - 1 - pos : 0];
                cs[j] = cpow[need ? r[j].w - r[j].z : 0];
            }
        }
        if (DECAY && lim < 4) {                              // pad lanes take no gradient
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (lim < 2) g[j].y = 0.f;
                if (lim < 3) g[j].z = 0.f;
                g[j].w = 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (r[j].x < 0) continue;
            if constexpr (DECAY) {
                a0 += (double)g[j].x * wd[j]; a1 += (double)g[j].y * wd[j]; a2 += (double)g[j].z * wd[j]; a3 += (double)g[j].w * wd[j];
            } else { a0 += g[j].x; a1 += g[j].y; a2 += g[j].z; a3 += g[j].w; }
            const int pos = base + sb + j, s = r[j].z, e = r[j].w;
            if (pos + 1 != e && pos + 1 != base + WCH) continue;       // the run goes on inside this chunk
            if (s >= base && e <= base + WCH) {                      // the whole segment lies in this chunk
                if constexpr (DECAY) {
                    *reinterpret_cast<float4*>(sa.table16 + (size_t)r[j].x * rw + 4 * q) =
                        make_float4((float)((double)wold[j].x * cs[j] - lr * a0), (float)((double)wold[j].y * cs[j] - lr * a1),
                                    (float)((double)wold[j].z * cs[j] - lr * a2), (float)((double)wold[j].w * cs[j] - lr * a3));
                } else {
                    float* dst = sa.table16 + (size_t)r[j].x * rw + 4 * q;
                    if (sa.tag_shared[r[j].x] == sa.stamp)
                        atomic_add4(dst, (float)(-lr * a0), (float)(-lr * a1), (float)(-lr * a2), (float)(-lr * a3));
                    else
                        *reinterpret_cast<float4*>(dst) =
                            make_float4((float)(wold[j].x - lr * a0), (float)(wold[j].y - lr * a1),
                                        (float)(wold[j].z - lr * a2), (float)(wold[j].w - lr * a3));
                }
            } else {
                const int which = (s < base) ? 0 : 1;                // 0: enters from the left; 1: opens here
                double* pp = sa.part + (((size_t)f * NQ + qc) * 2 + which) * rw + 4 * q;
                pp[0] = a0; pp[1] = a1; pp[2] = a2; pp[3] = a3;
                if (which == 1 && q == 0) sa.owners[atomicAdd(sa.owner_cnt, 1)] = make_int4(f, s, e, r[j].x);
            }
            a0 = a1 = a2 = a3 = 0;
        }
    }
}

// level 2: one workgroup per registered multi-chunk segment; groups of nq threads add the chunks' partials in a fixed order
template <bool DECAY>
__device__ __forceinline__ void scatw2_form(const ScatArgs& sa, const int blk, const int nblk, double* s_w /*[1024]*/)
{
    const int rw = sa.rw, nq = rw >> 2, NQ = sa.N2 / WCH, ngrp = 256 / nq;
    const int grp = threadIdx.x / nq, q = threadIdx.x % nq;
    const int n = *sa.owner_cnt;
    for (int o = blk; o < n; o += nblk) {
        const int4 ow = sa.owners[o];                      // {f, s, e, row}
        const int q0 = ow.y / WCH, q1 = (ow.z - 1) / WCH;
        double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        // the row (and its decay factor) is requested with the partial sums, not after them (one round trip less)
        float4* p = reinterpret_cast<float4*>(sa.table16 + (size_t)ow.w * rw + 4 * q);
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        double cdec = 0.0;                                 // DECAY only
        if (grp == 0) {
            w = *p;
            if constexpr (DECAY) cdec = sa.cpow[ow.z - ow.y];
        }
        if (grp < ngrp) {
            for (int qq0 = q0 + grp; qq0 <= q1; qq0 += 4 * ngrp) {           // four chunks' partials in flight at a time
                double v[4][4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int qq = qq0 + k * ngrp;
                    const double* pp = sa.part + (((size_t)ow.x * NQ + (qq <= q1 ? qq : q1)) * 2 + (qq == q0 ? 1 : 0)) * rw + 4 * q;
                    const bool on = qq <= q1;
                    v[k][0] = on ? pp[0] : 0.0; v[k][1] = on ? pp[1] : 0.0; v[k][2] = on ? pp[2] : 0.0; v[k][3] = on ? pp[3] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) { a0 += v[k][0]; a1 += v[k][1]; a2 += v[k][2]; a3 += v[k][3]; }
            }
            double* d = s_w + ((size_t)grp * nq + q) * 4;
            d[0] = a0; d[1] = a1; d[2] = a2; d[3] = a3;
        }
        __syncthreads();
        if (grp == 0) {
            double t0 = 0, t1 = 0, t2 = 0, t3 = 0;
            for (int gI = 0; gI < ngrp; ++gI) {
                const double* d = s_w + ((size_t)gI * nq + q) * 4;
                t0 += d[0]; t1 += d[1]; t2 += d[2]; t3 += d[3];
            }
            if constexpr (DECAY)
                *p = make_float4((float)((double)w.x * cdec - sa.lr * t0), (float)((double)w.y * cdec - sa.lr * t1),
                                 (float)((double)w.z * cdec - sa.lr * t2), (float)((double)w.w * cdec - sa.lr * t3));
            else if (sa.tag_shared[ow.w] == sa.stamp)
                atomic_add4(reinterpret_cast<float*>(p), (float)(-sa.lr * t0), (float)(-sa.lr * t1), (float)(-sa.lr * t2), (float)(-sa.lr * t3));
            else
                *p = make_float4((float)(w.x - sa.lr * t0), (float)(w.y - sa.lr * t1), (float)(w.z - sa.lr * t2),
                                 (float)(w.w - sa.lr * t3));
        }
        __syncthreads();
    }
}
__device__ __forceinline__ void scatw1_body(const ScatArgs& sa, const int blk) { scatw1_form<false>(sa, blk); }
__device__ __forceinline__ void scatw2_body(const ScatArgs& sa, const int blk, const int nblk, double* s_w) { scatw2_form<false>(sa, blk, nblk, s_w); }
__device__ __forceinline__ void scatdw1_body(const ScatArgs& sa, const int blk) { scatw1_form<true>(sa, blk); }
__device__ __forceinline__ void scatdw2_body(const ScatArgs& sa, const int blk, const int nblk, double* s_w) { scatw2_form<true>(sa, blk, nblk, s_w); }

static __global__ __launch_bounds__(256) void k_scatdw1(const ScatArgs sa) { scatdw1_body(sa, blockIdx.x); }
static __global__ __launch_bounds__(256) void k_scatdw2(const ScatArgs sa)
{
    __shared__ double s_w[1024];
    scatdw2_body(sa, blockIdx.x, gridDim.x, s_w);
}

// ------------------------------------------------------------------------------------------
// Host side: the buffers one grouping owns, the update's argument block, the plain launches.
// ------------------------------------------------------------------------------------------
// The buffers behind one grouping of N2 keys per field, and their one sizing rule (chunk = wide ? WCH : 16 sorted entries):
//   rec        F * N2 records {row, t, s, e}
//   part       two partial rows of rw doubles per chunk: F * (N2 / chunk) * 2 * rw
//   owners     a chunk opens at most one multi-chunk segment: F * (N2 / chunk) records -- on 16-float rows the F * N2 / 16 that
//              scat2w_form's speculative read rests on.  owners16: F * (N2 / 16) whatever the chunk, which is what the FM and
//              inner-product handles have always allocated on their wide paths too
//   owner_cnt  one int
// Zero-filled on `st`, like every other buffer of a handle.
struct RowGroupBufs { int4* rec = nullptr; double* part = nullptr; int4* owners = nullptr; int* owner_cnt = nullptr; };
inline hipError_t row_group_alloc(RowGroupBufs& b, int F, int N2, bool wide, int rw, hipStream_t st, bool owners16 = false)
{
    const size_t nchunk = (size_t)N2 / (wide ? WCH : 16);
    const size_t bytes[4] = {(size_t)F * N2 * sizeof(int4), (size_t)F * nchunk * 2 * rw * sizeof(double),
                             (size_t)F * (owners16 ? (size_t)N2 / 16 : nchunk) * sizeof(int4), sizeof(int)};
    void** const ptr[4] = {(void**)&b.rec, (void**)&b.part, (void**)&b.owners, (void**)&b.owner_cnt};
    for (int i = 0; i < 4; ++i) {
        hipError_t e = hipMalloc(ptr[i], bytes[i]);
        if (e == hipSuccess) e = hipMemsetAsync(*ptr[i], 0, bytes[i], st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
inline void row_group_free(RowGroupBufs& b)
{
    for (void* p : {(void*)b.rec, (void*)b.part, (void*)b.owners, (void*)b.owner_cnt}) if (p) hipFree(p);
    b = RowGroupBufs();
}

// Every field of the update's argument block.  What is no parameter starts as the plain update of 16-float rows has it -- no
// shared-row marks, one gradient row per example, level 2 by workgroup -- and is assigned by name where a site differs; `form`
// is set by scat1_blocks.
inline ScatArgs scat_args(const RowGroupBufs& b, int N2, int F, int K, const float* gxp, int K1p, const double* cpow, double lr,
                          float* table, int rw)
{
    return ScatArgs{b.rec, N2, F, K, gxp, K1p, cpow, lr, table, b.part, b.owner_cnt, b.owners, rw,
                    /*tag_shared*/ nullptr, /*stamp*/ 0, /*gxf*/ 0, /*form*/ SCAT1_QUARTER, /*form2*/ SCAT2_BLOCK};
}

// The split sort as plain launches on `st`: the runs alone (FM pre-training merges them beside its forward), or the runs and
// the rank merge.  4 so.F and 16 so.F workgroups; so.nblk belongs to the union launches.
// (Templates without a real parameter, these three: a unit instantiates the kernels they launch only if it calls them -- as
// plain inline functions they would put k_sortA / k_sortB / k_sort into the device code of every unit that includes this file.)
template <int = 0> void launch_sort_runs(hipStream_t st, bool key64, const SortArgs& so)
{
    if (key64) hipLaunchKernelGGL((k_sortA<unsigned long long>), dim3(4 * so.F), dim3(256), sortA_lds_bytes<unsigned long long>(so.merge4), st, so);
    else hipLaunchKernelGGL((k_sortA<unsigned>), dim3(4 * so.F), dim3(256), sortA_lds_bytes<unsigned>(so.merge4), st, so);
}
template <int = 0> void launch_sort(hipStream_t st, bool key64, const SortArgs& so)
{
    launch_sort_runs(st, key64, so);
    if (key64) hipLaunchKernelGGL((k_sortB<unsigned long long>), dim3(16 * so.F), dim3(256), sort_lds_bytes<unsigned long long>(), st, so);
    else hipLaunchKernelGGL((k_sortB<unsigned>), dim3(16 * so.F), dim3(256), sort_lds_bytes<unsigned>(), st, so);
}
// k_sort over N2 = 256 .. 16384 keys per field (a power of two): 4, 8 or 16 keys per thread
template <int = 0> void launch_k_sort(hipStream_t st, int N2, const int32_t* ids, int B, int F, int64_t n_rows, const RowGroupBufs& b,
                          const int32_t* extra, int n_extra, int* err)
{
    const int kpt = N2 <= 4096 ? 4 : (N2 == 8192 ? 8 : 16);
    const dim3 grid(F), blk(N2 / kpt);
    const size_t lds = (size_t)N2 * 8;
    if (kpt == 4) hipLaunchKernelGGL(k_sort<4>, grid, blk, lds, st, ids, B, F, n_rows, N2, b.rec, b.owner_cnt, extra, n_extra, err);
    else if (kpt == 8) hipLaunchKernelGGL(k_sort<8>, grid, blk, lds, st, ids, B, F, n_rows, N2, b.rec, b.owner_cnt, extra, n_extra, err);
    else hipLaunchKernelGGL(k_sort<16>, grid, blk, lds, st, ids, B, F, n_rows, N2, b.rec, b.owner_cnt, extra, n_extra, err);
}
// Both levels of the update of 16-float rows: level 1 in the form scat1_blocks settles on (call this after the last change to
// sa), then level 2 on nblk2 workgroups.
inline void launch_scat_narrow(hipStream_t st, ScatArgs& sa, int form, int nblk2)
{
    const int nblk1 = scat1_blocks(sa, form);
    hipLaunchKernelGGL(k_scat1, dim3(nblk1), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_scat2, dim3(nblk2), dim3(256), 0, st, sa);
}

}  // namespace fnn
