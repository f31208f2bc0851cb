/* dae_hip.h -- C ABI of the SNN-DAE pre-training kernels in libfnn_hip.so (MI355X, gfx950).
 *
 * Replaces the Theano denoising autoencoders of Atomu2014/deep-ctr's
 * python/sampling_based_denosing_autoencoder.py, as `get_da_weights` (:347-371) runs them
 * (batch_size = 1, corruption_level = 0, learning_rate = 0.1, tied weights, sigmoid, cross-entropy):
 *
 *   sparse_da   :234-345   one sampled negative per feature, rows gathered per example  -> dae_sparse_epoch
 *   da          :116-232   dense upper layers, online SGD                               -> dae_dense_epoch
 *   the lower-layer propagation inside da() :163-187                                   -> dae_bag_cumsum_sigmoid
 *                                                                           (+ rbm_affine / rbm_sigmoid)
 *   da          :116-232   the same with batch_size = M and a keep mask (corruption_level > 0)  -> dae_dense_batch
 * Both trainers are online (one example per step, every step reads what the previous one wrote):
 * ONE workgroup walks the examples in order.  Sampled negative ids are INPUTS (the reference draws
 * them from RandomState(123), :306); DEVICE pointers unless a parameter says "host".  Errors: the
 * FNN_ERR_* codes of fnn_hip.h; dae_last_error() has the message.
 */
#ifndef DAE_HIP_H
#define DAE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: what this header declares is what it exports */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

const char* dae_last_error(void);

/* One pass of sparse_da's loop over N examples (:295-332).  table [n_rows, H] f32 is CONSTANT: the
 * reference's `givens` makes the returned W the un-updated input, so only the biases learn.
 * idx [N, S] int32: the S sampled visibles of each example in line order (negative, positive, ...),
 * x [N, S] f32 their values; bhid [H] and bvis [S] (positional) are updated in place; bhid_prev [H]
 * receives bhid as it was BEFORE the last example's update (what the Theano call returns).
 * cost_sum_out (host, nullable): sum of the per-example costs.  H <= 256, S <= 32. */
int dae_sparse_epoch(const float* table, int64_t n_rows, float* bhid, float* bvis, float* bhid_prev,
                     const int32_t* idx, const float* x, int64_t N, int H, int S, float lr,
                     double* cost_sum_out, void* stream);

/* One pass of da()'s loop (:143-196) over X [N, row] f32 (already propagated through the lower
 * layers): W [row, col], bhid [col], bvis [row] updated in place by N online steps
 * W -= lr (x (x) dy + d (x) y).  skip_last_update != 0: the last example only contributes its cost
 * (the reference returns the parameters as they were before the last call's update).
 * W lives in the registers of one 1024-thread workgroup when [row][col] fits [304][128] or [208][320];
 * larger shapes (row <= 2048, col <= 1024) keep W in global memory. */
int dae_dense_epoch(float* W, float* bhid, float* bvis, const float* X, int64_t N, int row, int col,
                    float lr, int skip_last_update, double* cost_sum_out, void* stream);

/* Layer-0 propagation of da() (:166-187): out [n, H] = sigmoid(cumsum_k(sum of the rows W0[id] over
 * ALL ids of the example) + b0) -- the reference never resets its accumulator between hidden units,
 * so unit k receives the running sum over units 0..k.  ids [n, F] int32, -1 = none.  H <= 1024. */
int dae_bag_cumsum_sigmoid(const float* W0, const float* b0, int H, int64_t n_rows, const int32_t* ids,
                           int n, int F, float* out, void* stream);

/* The same three steps in float64 -- the reference's own precision (theano.config.floatX).  Its
 * lr = 0.1 online dynamics amplify a 1e-7 perturbation to O(1) within a few thousand steps at
 * 200/300/100 hidden units, so only an f64 run tracks the reference's trajectory end to end.  W of
 * the dense trainer stays in global memory here (any row <= 2048, col <= 1024); dae_dense_epoch
 * takes the same path for f32 shapes its register tilings do not hold. */
int dae_sparse_epoch_f64(const double* table, int64_t n_rows, double* bhid, double* bvis, double* bhid_prev,
                         const int32_t* idx, const double* x, int64_t N, int H, int S, double lr,
                         double* cost_sum_out, void* stream);
int dae_dense_epoch_f64(double* W, double* bhid, double* bvis, const double* X, int64_t N, int row, int col,
                        double lr, int skip_last_update, double* cost_sum_out, void* stream);
int dae_bag_cumsum_sigmoid_f64(const double* W0, const double* b0, int H, int64_t n_rows, const int32_t* ids,
                               int n, int F, double* out, void* stream);
/* out [n, b] = sigmoid(in [n, a] . W [a, b] + bias [b]): the propagation between dense layers (:183-187). */
int dae_affine_sigmoid_f64(const double* in, const double* W, const double* bias, int n, int a, int b,
                           double* out, void* stream);

/* da() as the reference writes it (:116-232), a MINI-BATCH trainer: one pass over X [N, row] in mini-batches of M
 * examples (batch_size, :162), a short last batch of N % M examples trained with its own mean (:196-228).  Per
 * mini-batch of m examples (dA.get_cost_updates, :97-113), every product reading W as it was at the batch's start:
 *   Xt = keep * X;  Y = sigmoid(Xt W + bhid);  Z = sigmoid(Y W^T + bvis);
 *   cost = mean_e -sum_i (X log Z + (1 - X) log(1 - Z))          against the UNcorrupted X (:104-105)
 *   D = (Z - X) / m;  dY = (D W) * Y (1 - Y);  W -= lr (Xt^T dY + D^T Y);  bhid -= lr sum_e dY;  bvis -= lr sum_e D
 * W [row, col], bhid [col], bvis [row] are updated in place.  keep [N, row] uint8, row-major like X: 0 = the input
 * is corrupted to 0, non-zero = kept (get_corrupted_input, :86-89); NULL = nothing corrupted, the same bits as an
 * all-ones mask.  The masks are INPUTS, like every random number of this header.  skip_last_update != 0: the last
 * mini-batch of the call contributes its cost only (the reference returns w, b as they were before the last
 * train_da call).  cost_sum_out (host, nullable): sum over the call's mini-batches of their mean cost, in f64 (the
 * caller divides by the number of mini-batches for :229's numpy.mean(c)).
 * Limits: N >= 1, 1 <= M <= 256, 1 <= row <= 512, 1 <= col <= 512; anything else, or a null W / bhid / bvis / X, is
 * FNN_ERR_ARG before any device call.  One persistent launch per call: eight workgroups, each with col / 8 columns
 * of W in registers, ONE hand-off between them per mini-batch (dae_dense_epoch_f64 makes one per example); a
 * workgroup that never arrives makes the call FNN_ERR_HIP.  The call allocates and frees its scratch (at most 25 MB).
 * Summation order (fixed: two calls on the same inputs give the same bits):
 *   X W, D W      per column: wave w adds rows w, w + 16, .. in that order (fma), then the 16 wave partials in wave order
 *   Y W^T         per row, over the 64 columns of a workgroup: f32 a butterfly (xor 1, 2, .. 32); f64 a fixed tree over
 *                 lanes 32, 16, .., 1 apart (the first steps move up to eight rows at once, a lane adding what it
 *                 receives to what it kept); then bvis + the eight workgroup partials in workgroup order
 *   W             the rank-1 terms lr (Xt[e] (x) dY[e] + D[e] (x) Y[e]) are subtracted example by example, e ascending
 *   bhid, bvis    the gradient is summed over the examples e ascending, then param -= lr * sum
 *   cost          f64: a thread of workgroup 0 adds its (e, i) terms of a batch (stride 1024 over e * RP + i within a sub-block of 4 (f64) or
 *                 8 (f32) examples, RP = 128 | 208 | 304 | 512, the smallest that holds row), sub-blocks ascending,
 *                 divides by m and adds that to its running sum; at the end a butterfly per wave, then the 16 waves in order
 * Not the reference's run: its products run in BLAS's order, and its corruption stream is Theano's (see the Python
 * module).  M = 1, keep = NULL computes dae_dense_epoch[_f64]'s step up to rounding, not bit for bit. */
int dae_dense_batch(float* W, float* bhid, float* bvis, const float* X, const uint8_t* keep,
                    int64_t N, int M, int row, int col, float lr, int skip_last_update,
                    double* cost_sum_out, void* stream);
int dae_dense_batch_f64(double* W, double* bhid, double* bvis, const double* X, const uint8_t* keep,
                        int64_t N, int M, int row, int col, double lr, int skip_last_update,
                        double* cost_sum_out, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DAE_HIP_H */
