// metrics.hip.h -- device-side evaluation metrics shared by the C ABIs (internal, not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <string>

#include "eval_group.h"

namespace fnn {
// AUC (ties at 1/2, the trapezoid of sklearn.metrics.roc_auc_score), RMSE and logloss
// (sklearn.metrics.log_loss: p clipped to [eps, 1 - eps], eps = 2^-52) of p [n] against labels
// y [n] (0 / non-zero), both DEVICE pointers.  out = {auc, rmse, logloss, n_pos}.  Synchronises `st`.
// Returns 0, -1 on a HIP error (err set), -2 when only one class is present (auc undefined; the
// other two are still written), -3 when any prediction is NaN or outside [0, 1] (err set to a message with
// their number; all three metrics are NaN, as roc_auc_score and log_loss raise ValueError on such input;
// this outranks -2).  y: 0 is the negative class, EVERY other int32 the positive one.
int device_metrics(hipStream_t st, const float* p, const int32_t* y, int64_t n, double out[4], std::string& err);

// Grouping of a GLOBAL batch for the exact data-parallel mode (fnn_step_scatter_global beyond the 16,384 keys the one-workgroup
// bitonic sort holds in LDS): per field f, the (row, t) pairs ids[t][f], t < B, sorted by (row, t) into
// rec[f * N2 + pos] = {row, t, s, e} -- [s, e) = the positions of the row's run inside the field -- and {-1, 0, 0, 0} for the
// N2 - (valid entries) slots that follow (ids outside [0, n_rows), t >= B).  N2 >= B, N2 <= 2^20.  The F * N2 64-bit keys are
// ordered by radix_sort_segments below (round 2 used rocPRIM here).  `ws` / `ws_bytes`: workspace owned by the caller,
// grown here when too small (hipMalloc: the first call synchronises).  Also zeroes *owner_cnt.  Returns 0 or -1 (err set).
int group_global(hipStream_t st, const int32_t* ids, int B, int F, int64_t n_rows, int N2, int4* rec, int* owner_cnt,
                 void** ws, size_t* ws_bytes, std::string& err);

// Stable LSD radix sort (8 bits per pass, bits [lo_bit, hi_bit)) of `nseg` independent segments of `n` 64-bit keys each
// (segment g = keys[g * n .. (g + 1) * n)), ping-ponging between `keys` and `tmp` (same size); `hist`: radix_sort_hist_bytes(nseg, n)
// bytes of workspace.  Enqueues 3 launches per pass on `st`; returns the buffer that holds the result.  Stable: keys that agree on
// the sorted bits keep their order -- generate keys in arrival order and sort on the row bits alone.
unsigned long long* radix_sort_segments(hipStream_t st, unsigned long long* keys, unsigned long long* tmp, unsigned* hist, int nseg, int n,
                                        int lo_bit, int hi_bit);
size_t radix_sort_hist_bytes(int nseg, int n);
// The same sort over 32-bit keys (the metric keys `label << 31 | bits of p`: half the traffic of the 64-bit form).
uint32_t* radix_sort_segments32(hipStream_t st, uint32_t* keys, uint32_t* tmp, unsigned* hist, int nseg, int n, int lo_bit, int hi_bit);

// device_metrics for the predictions of `nseg` models on ONE feed, p [nseg][n] against the one y [n], without rocPRIM, without an
// allocation and without a synchronisation: everything is enqueued on `st` and out[m] (DEVICE, [nseg]) receives what model m's
// metrics are made of.  The partition of the sums is device_metrics' -- 2,048 examples a block, its tree, the block partials added
// in block order in f64 -- and the AUC's sum is an integer, so
//     auc = auc_sum / (2 n_pos n_neg),  rmse = sqrt(se / n),  logloss = ll / n
// are bit for bit what device_metrics returns for p[m].  n_bad != 0: model m has predictions NaN or outside [0, 1] (-3 there).
// n_pos (DEVICE, one count): written when count_pos != 0 -- y is shared, so the first call over a feed counts and the later
// ones (further groups of models) read it; the AUC pass takes n_neg from it on the device.  One class only: auc_sum stays 0.
// scratch: metrics_multi_bytes(nseg, n) bytes, about 8.5 n per model; 1 <= n <= 2^30.
// (struct MetricOut { double se, ll; unsigned long long auc_sum, n_bad; }: eval_group.h)
size_t metrics_multi_bytes(int nseg, int64_t n);
hipError_t metrics_multi(hipStream_t st, const float* p, const int32_t* y, int64_t n, int nseg, void* scratch, int count_pos,
                         unsigned long long* n_pos, MetricOut* out);

// ---- evaluating many models on one feed: what fm_eval_multi, fnn_eval_multi and ipnn_eval_multi share (DESIGN.md section 4,
// "The group calls' shared host side").  The models go in groups of G, each group through one scratch allocation.
// The scratch of a group of G models on N lines, carved from `base` in pieces of up256(): the predictions p [G][N], the metric
// pass's own scratch, out [G], the range flags [G] and the feed's count of positives.
struct EvalScratch {
    float* p; void* metric; MetricOut* out; int* flags; unsigned long long* n_pos;
    EvalScratch(int G, int64_t N, char* base);
    static size_t bytes(int G, int64_t N);
};
// The group size of a call on n_models: as many as fit EvalScratch::bytes under $cap_env (default 2^30), one at the least.
int eval_group_size(int n_models, int64_t N, const char* cap_env);
// Where the metrics go ([n_models] each, any of them null) and, where given, the predictions (p_out null, or DEVICE [N] / null each).
struct EvalOut { double *auc, *rmse, *logloss; int* status; float* const* p_out; };
// What the verdict (eval_verdict) is made of: the models with bad predictions, those with ids out of range, the feed's positives.
struct EvalFound { std::string bad, range; unsigned long long n_pos = 0; };
// The loop over the groups of G on stream `st`, `scratch` (DEVICE, EvalScratch::bytes(G, N)) the caller's.  Per group of members
// g0 .. g0 + n:  forward(g0, n, p) launches their predictions into p[0 .. n) and flags(g0, n, flags_d) the family's kernel that
// reads (and clears) their range flags into flags_d[0 .. n) -- both return FNN_OK or the failure's code, its text left where the
// family leaves it; then metrics_multi (which counts the positives in the first group only), the copies to out.p_out, the copies
// home and the group's ONE synchronisation, after which out and `found` take the group's results.  A HIP error of the loop's own
// returns FNN_ERR_HIP with its text in `err`.  On every error return the stream has been synchronised: nothing still uses the
// scratch, which the caller may free or reuse at once.
using EvalForward = std::function<int(int g0, int n, float* const* p)>;
using EvalFlags = std::function<int(int g0, int n, int* flags_d)>;
int eval_groups(hipStream_t st, int n_models, int G, const int32_t* y, int64_t N, char* scratch, const EvalForward& forward,
                const EvalFlags& flags, const EvalOut& out, EvalFound& found, std::string& err);

// Sorted keys `row << 20 | index` (row = 2^31 - 1: invalid, sorted last) of `nseg` segments of `n` -> rec[g * n + pos] =
// {row, index, s, e}, [s, e) = the positions of the row's run inside its segment; {-1, 0, 0, 0} for invalid entries.
constexpr int GROUP_INDEX_BITS = 20;
constexpr unsigned long long GROUP_INVALID_ROW = (1ull << 31) - 1;
void group_records(hipStream_t st, const unsigned long long* sorted, int nseg, int n, int4* rec);
}  // namespace fnn
