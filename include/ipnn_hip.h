/* ipnn_hip.h -- C ABI of the inner-product FNN family (FNN_IP_L3 / L5 / L7) in libfnn_hip.so.
 *
 * Replaces the TensorFlow graph of Atomu2014/deep-ctr's python/FNN_IP_L7.py (and _L3 / _L5, same
 * pattern): `forward` :102-133 (embeddings, pair-wise inner products, z1 = [e | p | b], then
 * l_{t+1} = dropout(act(l_t)) W_t + b_t with activation and inverted dropout BEFORE every matmul),
 * the loss sum(sigmoid_cross_entropy_with_logits) :82-88 and the gradient step.  One id per field, and -- through the
 * `_w` entry points -- one value weight per (example, field): e_f = wts[t][f] * table[ids[t][f]], which is both the iPinYou
 * shape (every weight 1) and the reference's Criteo feed (13 numeric fields `v_wt * fm_wv[i]`, :103, and 26 weighted categorical
 * ones).  Optimiser: plain SGD, Adam or FTRL (IPNN_OPT_*).  Dropout keep-masks are INPUTS (uint8, one per element,
 * reference column order), NULL = no dropout (`drop_out=False`) -- or DRAWN by the library from (seed, step):
 * ipnn_train_step_drawn, the same step without the caller's mask arrays (ipnn_draw_masks writes the masks it draws).
 *
 * Field counts: narrow rows (k = 1..16) take 2..64 fields -- the reference's classes are 39-field models (X_feas = 13 +
 * len(cat_sizes), python/FNN_IP_L3.py) -- with and without `pairs`, in both precisions, under every optimiser; layer 0 then holds
 * 16 F + F(F-1)/2 + 2 columns padded to a multiple of 64: at most 3072 (64 fields with pairs; 1408 at 39).  Up to 32 fields the
 * inner-product layer runs 16 examples per workgroup; above, 8 (forward) and 4 (backward) with only the embeddings in LDS.  The
 * deep stack runs on the strip kernels -- a strip of examples through every product inside one workgroup, the activations in two
 * LDS tiles -- while the tiles fit: up to 32 fields two equal tiles of at most 1024 columns; above, with a layer 0 wider than
 * that, two tiles of the widths each launch's layers need, 2560 columns together (every stack of the reference at its 39 fields;
 * not 64 fields with pairs, not FNN_IP_L7 from 43 fields on).  Otherwise one GEMM launch per product.  ipnn_plan_query tells, and
 * IPNN_STRIP_L0=0 in the environment of ipnn_create keeps the limit of 1024 columns for every handle.  Wide rows stay at 2..32
 * fields.
 *
 * Wide rows (k = 17..128, any of 2..32 fields, both `pairs`, both precisions, every optimiser): the table keeps rows of
 * rw = rup(k, 4) floats (pad columns zero; under Adam / FTRL the state and gradient tables are [n_rows, rw] too) and layer 0
 * holds column f*rw + l = e_f[l], then the pair products, b and the ones column: rup(F*rw + P + 2, 64) padded columns (at most
 * 4608: 32 fields of 128).  The layout is internal: every entry point below takes and returns the reference's shapes.
 *
 * Error codes are the FNN_ERR_* of fnn_hip.h; ipnn_last_error() has the message.
 */
#ifndef IPNN_HIP_H
#define IPNN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: what this header declares is what it exports */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define IPNN_ACT_TANH    0      /* python/tf_util.py:32-38 `activate` */
#define IPNN_ACT_SIGMOID 1
#define IPNN_ACT_RELU    3

#define IPNN_MAX_HIDDEN  8

#define IPNN_OPT_SGD     0      /* python/tf_util.py:26-29 GradientDescentOptimizer                       */
#define IPNN_OPT_ADAM    1      /* python/tf_util.py:17-20 AdamOptimizer(learning_rate, epsilon): the
                                   reference's choice for this family (python/baseline.py:146, lr 1e-4,
                                   eps 1e-8).  TensorFlow's gradient of the embedding tables is dense, so
                                   EVERY row's moments decay and every row moves each step             */
#define IPNN_OPT_FTRL    2      /* python/tf_util.py:21-24 FtrlOptimizer(learning_rate): TensorFlow's
                                   defaults (learning_rate_power -0.5, initial accumulator 0.1, l1 = l2 =
                                   0); also a dense pass over the tables: a row no example has touched is
                                   re-derived from its (zero) linear term, i.e. drops to 0 at step 1   */

typedef struct ipnn_cfg {
    int32_t n_fields;                  /* X_feas: 2..64 with k <= 16, 2..32 with k = 17..128 */
    int32_t k;                         /* rank + 1: embedding row [w | v]  (FNN_IP_L7.py:66); 1..128:
                                          k <= 16 keeps rows in 16-float slots; k = 17..128 (the FM50 /
                                          FM100 seeds) is the WIDE layout below                */
    int32_t n_hidden;                  /* 3, 5 or 7 (any 1..8)                               */
    int32_t hidden[IPNN_MAX_HIDDEN];   /* e.g. 1000,800,600,400,200,100,50 (baseline.py:139) */
    int32_t act;                       /* IPNN_ACT_*                                         */
    int32_t pairs;                     /* 1: z1 = [e | p | b] (FNN_IP_L*, FNN_IP_L7.py:108-114);
                                          0: z1 = [e | b], the plain `FNN` class (python/FNN.py:80) */
    int32_t max_batch;                 /* <= 4096                                            */
    int32_t precision;                 /* FNN_PREC_F32 / FNN_PREC_BF16                       */
    float   lr;
    float   keep_prob;                 /* _reg_argv[0]                                       */
    int32_t optimizer;                 /* IPNN_OPT_*                                         */
    float   adam_beta1, adam_beta2;    /* TensorFlow defaults 0.9, 0.999                     */
    float   adam_eps;                  /* _ptmzr_argv[2]                                     */
    int32_t device;
    void*   stream;
} ipnn_cfg;

typedef struct ipnn_handle ipnn_handle;

const char* ipnn_last_error(const ipnn_handle* h);
/* sizeof(ipnn_cfg) as the library was compiled (a binding checks its own struct against it). */
uint64_t ipnn_cfg_size(void);
int ipnn_create(const ipnn_cfg* cfg, ipnn_handle** out);

/* What ipnn_create would choose for a cfg under the environment's knobs, computed without a device (and without a handle): the
 * code ipnn_create itself runs.  cfg's device and stream are not read.  A cfg that ipnn_create refuses for its shape is refused
 * here with the same message (ipnn_last_error(NULL)).
 *   A strip launch keeps a strip's activations in two LDS tiles, A and B, which alternate from layer to layer; cap_a / cap_b are
 * their widths in padded columns (the widest layer that lands in each over the launch's range) and lds_bytes the launch's dynamic
 * LDS.  The launches: the whole stack forward and backward (one launch per direction: every f32 step, a bf16 batch too long for
 * pairs, every group call), the wide range forward and backward (products 1 .. cut, as pairs of workgroups) and the narrow tail
 * (products cut + 1 .. n_hidden + 1) forward, backward and fused (both in one launch: the default form of a bf16 training step
 * that splits).  Launches a handle never issues are all zero: every one on the GEMM path, the last five where 1 <= cut < n_hidden
 * does not hold. */
#define IPNN_ROWS_NARROW 0      /* 16 examples per workgroup (k_ip_fwd / k_ip_bwd)                         */
#define IPNN_ROWS_WIDE   1      /* k = 17..128                                                             */
#define IPNN_ROWS_MANY   2      /* 33..64 fields: 8 examples forward / 4 backward, the embeddings in LDS   */
typedef struct ipnn_tiles { int32_t cap_a, cap_b; uint64_t lds_bytes; } ipnn_tiles;
typedef struct ipnn_plan_info {
    int32_t strips;                        /* 1: the strip kernels run the deep stack; 0: one GEMM launch per product */
    int32_t pairs;                         /* 1: batches whose pairs fit the chip run two workgroups per strip (bf16)  */
    int32_t cut;                           /* products 1 .. cut are wide enough for pairs                             */
    int32_t rows_fwd, rows_bwd;            /* IPNN_ROWS_*: the inner-product layer's kernels, per direction           */
    int32_t shares_step, shares_eval;      /* 1: the handle shares the launches of ipnn_train_step_multi / of
                                              ipnn_predict_multi and ipnn_eval_multi; 0: it runs its own inside them  */
    int32_t n_layers;                      /* n_hidden + 2                                                            */
    int32_t padded[IPNN_MAX_HIDDEN + 2];   /* padded width of layer 0 .. n_hidden + 1                                 */
    ipnn_tiles stack_fwd, stack_bwd, wide_fwd, wide_bwd, tail_fwd, tail_bwd, tail_fused;
    uint64_t lds_max;                      /* the largest lds_bytes above                                             */
} ipnn_plan_info;
/* sizeof(ipnn_plan_info) as the library was compiled */
uint64_t ipnn_plan_info_size(void);
int ipnn_plan_query(const ipnn_cfg* cfg, ipnn_plan_info* out);

int ipnn_destroy(ipnn_handle* h);
int ipnn_sync(ipnn_handle* h);

/* HOST pointers.  table rows [n_rows, K] = concat(W, V) (fm_wv, :66); b: the scalar `fm_b`.
 * Under Adam / FTRL, ipnn_set_table restarts the optimiser as fm_set_table does: the state of the table, of every dense layer
 * and of b goes back to what ipnn_create left (Adam: m = v = 0; FTRL: accum = 0.1, linear = 0) and the step count to 0; n_rows
 * may differ from the last call's.  ipnn_set_layer and ipnn_set_b replace values only and leave the optimiser's state alone. */
int ipnn_set_table(ipnn_handle* h, const float* rows, int64_t n_rows);
int ipnn_get_rows(ipnn_handle* h, const int64_t* row_ids, int64_t n, float* out);
int ipnn_set_b(ipnn_handle* h, float b);
int ipnn_get_b(ipnn_handle* h, float* b);
/* layer i = 1 .. n_hidden+1: W [d_{i-1}, d_i], bias [d_i]; d_0 = F*K + F(F-1)/2 + 1 (`mbd_dim`,
 * FNN_IP_L3.py:18), d_{n_hidden+1} = 1.  Reference row order of h1_w: [e_0..e_{F-1} | pairs | b]. */
int ipnn_set_layer(ipnn_handle* h, int layer, const float* W, const float* bias);
int ipnn_get_layer(ipnn_handle* h, int layer, float* W, float* bias);

/* DEVICE pointers: ids int32 [B, F], y f32 [B], masks[t] uint8 [B, d_t] for t = 0..n_hidden
 * (array of n_hidden+1 device pointers held in HOST memory; NULL = no dropout).
 * One SGD step.  logits_out [B] (device, nullable); loss_sum_out (host, nullable: synchronises). */
int ipnn_train_step(ipnn_handle* h, const int32_t* ids, const float* y, int B,
                    const uint8_t* const* masks, float* logits_out, float* loss_sum_out);
/* Loss reduction of the following train steps: 0 (default) = tf.reduce_sum, 1 = tf.reduce_mean over the batch
 * (`_ptmzr_argv[-1]`, python/FNN_IP_L7.py:83-86): every gradient of a step is scaled by 1 / B.  loss_sum_out stays the
 * SUM of the per-example cross-entropies (divide by B on the host for the mean). */
int ipnn_set_loss_mean(ipnn_handle* h, int mean);
/* p_out [B] = sigmoid(logits) without dropout (`test_preds`, FNN_IP_L3.py:81-84). */
int ipnn_predict(ipnn_handle* h, const int32_t* ids, int B, float* p_out);

/* Value weights: the same three calls with wts f32 [B, F] (DEVICE pointer, row-major like ids): the embedding of field f of
 * example t is e_f = wts[t][f] * table[ids[t][f]] (python/FNN_IP_L7.py:103 for the numeric fields, the c_wts of
 * embedding_lookup_sparse for the categorical ones); pairs, z1, the stack and the loss follow from e, and the gradient of a row
 * is wts[t][f] * dL/de_f.  wts == NULL means every weight 1 and IS the call without `_w` (which forwards here with NULL): the
 * same kernels, bit-identical results.  Weights are data: they are not range-checked, zero and negative values are legal (a
 * zero weight leaves its row's gradient exactly 0), NaN and Inf propagate into the outputs and the touched rows.
 * ipnn_eval_w advances wts with ids, max_batch examples a chunk. */
int ipnn_train_step_w(ipnn_handle* h, const int32_t* ids, const float* wts, const float* y, int B,
                      const uint8_t* const* masks, float* logits_out, float* loss_sum_out);
int ipnn_predict_w(ipnn_handle* h, const int32_t* ids, const float* wts, int B, float* p_out);

/* Drawn keep-masks: a training step whose masks the library draws itself, a pure function of (seed, step, layer t, example ex,
 * column c) -- c in the reference column order of `masks`, layer 0 = [e | pairs | b] -- so that two integers reproduce a step:
 *     Philox4x32-10 (Salmon et al., Random123: multipliers 0xD2511F53 / 0xCD9E8D57, key bumps 0x9E3779B9 / 0xBB67AE85, ten rounds)
 *     key     = (lo32(seed), hi32(seed))
 *     counter = (c, (t << 16) | (ex >> 2), lo32(step), hi32(step));   word j (0..3) of the output belongs to example 4 (ex >> 2) + j
 *     keep    = word < min(2^32 - 1, floor((double)keep_prob * 2^32));   keep_prob >= 1: every element is kept
 * seed and step: any uint64.  The mask of an element depends on neither B nor d_t.  ipnn_train_step_drawn(seed, step) is
 * bit-identical (logits, loss, every parameter) to ipnn_train_step_w given the arrays ipnn_draw_masks(seed, step) wrote; wts is
 * nullable as there.  deep-ctr_amd/dropout.py restates the draw in NumPy. */
/* one training step whose keep-masks the library draws itself (above); wts nullable as in ipnn_train_step_w */
int ipnn_train_step_drawn(ipnn_handle* h, const int32_t* ids, const float* wts, const float* y, int B,
                          uint64_t seed, uint64_t step, float* logits_out, float* loss_sum_out);
/* the masks that call draws, in the ABI's layout: masks_out = n_hidden+1 DEVICE pointers held in HOST memory,
   uint8 [B, d_t] each (a NULL entry is skipped); on the handle's stream */
int ipnn_draw_masks(ipnn_handle* h, uint64_t seed, uint64_t step, int B, uint8_t* const* masks_out);

/* Evaluation pass (python/baseline.py:382-437 `test`): predict all N examples (DEVICE ids [N, F]
 * int32, y [N] int32; chunks of max_batch), then AUC / RMSE / logloss on the device.  Metrics are
 * HOST doubles.  y: 0 / non-zero.  One class only: FNN_ERR_RANGE (rmse and logloss are still written).  Any prediction NaN or
 * outside [0, 1] (a diverged model): FNN_ERR_RANGE, all three metrics NaN, their number in ipnn_last_error. */
int ipnn_eval(ipnn_handle* h, const int32_t* ids, const int32_t* y, int64_t N, double* auc, double* rmse, double* logloss);
int ipnn_eval_w(ipnn_handle* h, const int32_t* ids, const float* wts, const int32_t* y, int64_t N,
                double* auc, double* rmse, double* logloss);

/* Many models on ONE feed in one call (a hyper-parameter search scoring its candidates; DESIGN.md section 4, "Evaluating many
 * inner-product models").  hs, auc, rmse, logloss, status and p_out are HOST arrays of n_models entries (each output array may be
 * NULL); ids [N, F] int32, wts [N, F] f32 (nullable: every weight 1, as in ipnn_predict_w), y [N] int32 and every p_out[m] [N] are
 * DEVICE pointers; 1 <= N <= 2^30, not bounded by any member's max_batch.  p_out[m] is required in ipnn_predict_multi; in
 * ipnn_eval_multi an entry may be NULL.
 *   Results: p_out[m] is bit for bit what ipnn_predict_w(hs[m], ..) writes when called in chunks of that handle's max_batch;
 * auc[m], rmse[m], logloss[m] are bit for bit what ipnn_eval_w(hs[m], ..) returns.  status[m] is FNN_OK, or FNN_ERR_RANGE for a
 * model with a prediction NaN or outside [0, 1]: its three metrics are NaN, every other model's results stand.  Only one class in
 * y: every auc[m] is NaN, rmse and logloss are written.  An id outside [0, n_rows) is judged per model (table sizes may differ):
 * ipnn_eval_multi reports those models and clears their flags, ipnn_predict_multi leaves them to each handle's ipnn_sync.  Any of
 * the three makes the call return FNN_ERR_RANGE with the models' indices in ipnn_last_error(hs[0]); every other result is written.
 *   The calls only read the models, and may be interleaved with every other call on the members.  Each member's pending work
 * (the deferred dense update and sparse-row chain of IPNN_UPDATE_SIDE=1) is joined first; everything then runs on hs[0]'s stream,
 * which first waits for every other member's streams, and they wait for the call's last launch.  Members whose prediction runs
 * on the strip kernels share launches: per feed batch (as many lines as the smallest member's buffers hold: at most 4096, a
 * multiple of 256) and LAUNCH CLASS -- element type, n_hidden, the padded widths, the gather's row kind, pairs, weights given
 * or not; activation, k, table size and values may differ -- one inner-product launch and one launch over the whole stack,
 * both with the model as a grid dimension, one workgroup per strip (no workgroup of a group launch waits for another).  The
 * other members (a stack too wide for the strips' tiles, IPNN_STRIP=0) run their own launches inside the call.  ipnn_eval_multi takes
 * the models in groups of as many as fit $IPNN_EVAL_SCRATCH_BYTES (read per call, default 2^30, one model at the least; N * 4
 * bytes of predictions plus the metric pass's ~8.5 N per model) in one allocation hs[0] keeps while it is large enough; each
 * group costs one metric pass and one synchronisation.  Neither where the feed nor where the groups are cut changes a bit.
 * ipnn_predict_multi allocates nothing after hs[0]'s first group call and does not synchronise.
 *   Refusals (nothing launched, nothing written; the message starts with the function's name, names the offending model and is
 * left with ipnn_last_error(hs[0]), or ipnn_last_error(NULL) without a usable hs[0]): FNN_ERR_ARG for null hs, a null entry,
 * n_models outside 1..IPNN_EVAL_MAX_MODELS, null ids / y / p_out (or a null entry of it, predict), N out of range, n_fields or
 * device differing from hs[0]'s, a handle listed twice (its own a[0] buffer is the group launch's scratch); FNN_ERR_STATE for a
 * handle without a table.  n_models == 1 is accepted: the group path was measured not faster there (profiles/
 * ipnn_eval_multi_bench.json), so it runs the solo launches of ipnn_predict_w / ipnn_eval_w and reports as the group path does. */
#define IPNN_EVAL_MAX_MODELS 1024
int ipnn_predict_multi(ipnn_handle* const* hs, int n_models, const int32_t* ids, const float* wts,
                       int64_t N, float* const* p_out);
int ipnn_eval_multi(ipnn_handle* const* hs, int n_models, const int32_t* ids, const float* wts,
                    const int32_t* y, int64_t N, double* auc, double* rmse, double* logloss,
                    int* status, float* const* p_out);

/* One mini-batch step of many models on ONE feed in one call (a hyper-parameter search training its candidates; DESIGN.md
 * section 4, "A mini-batch step for many inner-product models"): one ipnn_train_step_w or ipnn_train_step_drawn of every handle
 * of the list.  ids [B, F] int32, wts [B, F] f32 (nullable: every weight 1) and y [B] f32 are DEVICE pointers; hs, masks, seeds,
 * steps, logits_out and loss_sum_out are HOST arrays of n_models entries.  masks[m] is what ipnn_train_step_w takes for model m
 * (L + 1 device pointers; a NULL entry: no dropout for that model); seeds[m] / steps[m] are what ipnn_train_step_drawn takes for
 * model m.  masks and seeds both NULL: no dropout anywhere; both given: refused.  logits_out is nullable and so are its entries
 * (device, [B] each).  loss_sum_out is nullable: when given it receives every model's loss sum through ONE packed device-to-host
 * copy and ONE synchronisation for the whole call.
 *   Contract: after the call every model's table rows, b, dense layers, optimiser state, Adam step count, logits_out[m] and
 * loss_sum_out[m] are bit for bit what that handle's own solo call would have left.  Group steps, solo steps, predict, evaluate,
 * the _multi evaluation calls, ipnn_set_* and ipnn_get_* interleave freely.  SGD, Adam and FTRL members may be mixed, and so may
 * act, k, pairs, depths, widths, table sizes, lr, keep_prob, the mean / sum loss and both precisions.  A member's pending
 * IPNN_UPDATE_SIDE=1 update is joined first; everything then runs on hs[0]'s stream, which first waits for every other member's
 * stream, and they wait for the call's last launch.
 *   Members on the strip kernels with narrow rows (k <= 16, any field count) share launches: per LAUNCH CLASS -- the
 * prediction launch class of ipnn_predict_multi plus the split-K layout of the weight gradients -- every stage of the step runs
 * ONCE with the model as a grid dimension (b and the table pass of an Adam / FTRL member are that member's own two launches), one workgroup per strip (no pair form, no tail split: no workgroup of a group launch
 * waits for another).  Members that agree in n_rows, key width and sort runs share one grouping of the batch's ids.  Every other
 * member (wide rows, a stack too wide for the strips' tiles, IPNN_STRIP=0, IPNN_GROUP_WGRAD=0, a diagnostic knob) runs
 * its own solo step inside the call: no shape is refused.  n_models == 1 forwards to the solo step.
 *   Refusals (before any launch and any write; the message starts with the function's name, names the model and is left with
 * ipnn_last_error(hs[0]), or ipnn_last_error(NULL) without a usable hs[0]): FNN_ERR_ARG for null hs or a null entry, n_models
 * outside 1..IPNN_STEP_MAX_MODELS, null ids or y, B < 1 or above a member's max_batch, n_fields or device differing from model
 * 0's, a handle listed twice (it is written to), masks and seeds both given, seeds without steps or steps without seeds, a
 * masks[m] with a null layer entry; FNN_ERR_STATE for a member without a table or one whose strip pair gave up earlier.  A
 * member's step count and pending flags are committed only after the call's last launch was accepted.
 *   An id outside a member's table behaves as in the solo step (the row reads as zero, the member's range flag is set).  With
 * loss_sum_out the call then returns FNN_ERR_RANGE, names the models whose flag was set and clears those flags, as
 * ipnn_eval_multi does; without it the flags stay for each handle's ipnn_sync.  A member that runs its own step inside the call
 * and whose strip pair gave up is judged as ipnn_sync judges it after a solo step: with loss_sum_out the call returns
 * FNN_ERR_HIP naming the model, its flag is cleared and the handle refuses further train steps. */
#define IPNN_STEP_MAX_MODELS 256
int ipnn_train_step_multi(ipnn_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const float* y, int B,
                          const uint8_t* const* const* masks, const uint64_t* seeds, const uint64_t* steps,
                          float* const* logits_out, float* loss_sum_out);

/* Measurement hook (bench.py): HIP events on the handle's stream around the segments of a train
 * step -- "mask_t" (the keep-masks: transposed, or drawn), "sort", "ip_fwd", "fwd", "bwd", "wgrad", "ip_bwd", "scatter", "update".  enable(1) clears
 * earlier samples; get returns the average device time of one segment in ms (0 if none). */
int ipnn_prof_enable(ipnn_handle* h, int on);
int ipnn_prof_get(ipnn_handle* h, const char* which, double* avg_ms);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* IPNN_HIP_H */
