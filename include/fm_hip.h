/* fm_hip.h -- C ABI of factorisation-machine pre-training in libfnn_hip.so (MI355X, gfx950).
 *
 * The step BEFORE the FNN hot path: the model whose rows [w_i, v_i1..v_ik]
 * `fm.model.txt` carries into python/FNN_wnzh.py:62-84.  Arithmetic of the reference's TensorFlow
 * class python/FM.py: `factorization` :55-64
 *      yhat = b + sum_i w_i x_i + 1/2 (|sum_i v_i x_i|^2 - sum_i |v_i|^2 x_i^2),
 * loss :36-41 (sigmoid cross-entropy, reduce_sum or reduce_mean, + lambda * (l2_loss(W) + l2_loss(V)
 * + l2_loss(b)) with tf.nn.l2_loss = sum(t^2)/2), plain SGD (python/tf_util.py:26-29), as driven by
 * python/ipinyou.py:136-173.  One feature per field: ids [B, F] int32 with -1 = absent.  Its value x is 1 (iPinYou;
 * `load_ipinyou_data` returns X_val = 1) through fm_train_step / fm_predict / fm_eval, or wts[t][f] through the *_w entry points
 * (the reference's `sp_wt_hldr`, python/FM.py:24-29 and python/LR.py:23-27; python/baseline.py:345 feeds the values of Criteo's 13
 * numeric fields and the weights of its 26 categorical ones).  With e_f = x_f * row(ids[t][f]):
 *      yhat = b + sum_f e_f[0] + 1/2 (sum_l (sum_f e_f[l])^2 - sum_f sum_l e_f[l]^2),
 *      d yhat / d w_f = x_f,   d yhat / d v_f[l] = x_f (S_l - e_f[l]),   S_l = sum_f e_f[l];
 * (x v)^2 is the reference's v^2 x^2 up to f32 rounding.  Weights are data and are not range-checked: zero and negative ones are
 * legal, a zero weight adds exactly 0 to its row's gradient (the row is still stamped for Adam / FTRL), NaN / Inf at a present
 * field propagate, and the weight of an absent field (id = -1) has no effect whatever its value.
 *
 * Ranks 0..127 (k = rank + 1 = 1..128: python/baseline.py's FM10, FM50 and FM100), 1..64 fields (python/baseline.py's
 * 39-column runs included), batches up to 4096.
 * Row layout on the device: k <= 16 keeps the FNN path's 64-byte rows (16 floats; in the forward a lane per field up to 16
 * fields, beyond that lane f takes fields f, f + 16, ..); k >= 17 takes the wide path, rows of rup(k, 4) floats (k = 101: 104)
 * so that every row piece is one 16-byte access, a half or quarter wave per example in the forward, 16 fields at a time.  The
 * library picks the layout from k; padding columns are zero and stay zero.  The host sees [n_rows, k] either way.
 *
 * Columns and rows.  The update groups a batch's entries per column ("field"): inside a column, repeated rows sum their
 * gradients in example order (f64) and the row takes one rounded store.  By default a row id must belong to ONE column of a
 * batch (iPinYou with a field per column: every field owns its own range of ids); a row under two columns would be updated by two
 * unordered read-modify-writes in one launch and could lose one of them (not checked).  fm_set_shared_rows(h, 1) lifts this:
 * columns are then mere positions, as in the reference, whose classes have no fields (python/FM.py:23-29 takes batch_size *
 * X_feas (id, weight) pairs and embedding_lookup_sparse sums whatever it is given; python/ipinyou.py:42-65 lists a line's
 * features in line order, so a missing field shifts the rest one column left and a multi-valued field takes several).  With the
 * mode on, a training step is correct for ANY ids in [-1, n_rows), all optimisers, both layouts, with or without weights:
 *   - a row under several columns of a batch receives every column's contribution; a row twice on one line is two columns;
 *   - a row held by one column of the batch takes the same single rounded store as with the mode off, and a batch in which no
 *     row is shared leaves table, bias and optimiser state bit-identical to the mode being off;
 *   - a shared row receives one f32 atomic add per (column, segment) of that segment's f64 sum (SGD: into the row, under the
 *     lazy scale; Adam / FTRL: into the zeroed gradient store), in no fixed order: such rows are reproducible to f32 rounding,
 *     not bit for bit (a bit-reproducible form would need a second grouping across columns);
 *   - the narrow rows (k <= 16) run the half-chunk level 1 and the wave-per-segment level 2 of the sparse-row update in their
 *     shared-row forms whatever FNN_SCAT1_FORM / FNN_SCAT2_FORM say.
 * With the mode off nothing changes.  Predictions, the loss, fm_predict* and fm_eval* are exact for any ids in either mode.
 * Of the ranks, only 15 (k = 16) does not feed the FNN step: fnn_create refuses k = 16 (its other limits: fnn_hip.h).
 *
 * The L2 term makes TensorFlow's gradient DENSE: every step multiplies the whole table by
 * (1 - lr * lambda).  Here the table is kept as `scale * stored` -- the decay is one scalar
 * multiplication per step, touched rows get -lr * g / scale through the same sorted, atomics-free
 * sparse-row update as the FNN path, and the scale is folded back into the rows before it leaves
 * 2^-24 .. 1.  Same result as the dense update up to f32 rounding.
 *
 * Adam and FTRL (python/tf_util.py:15-24, fm_set_optimizer): the lazy scale cannot express them -- under Adam every row's
 * moments decay each step, under FTRL every variable is re-derived from its linear term.  The batch's per-row gradient sums
 * then go into a zeroed gradient store instead of the table, and one streaming pass over every live element (row < n_rows,
 * column < k) applies g = G + lambda * w, the optimiser and its state, and clears G.  The state is compact [n_rows, k].
 * With k = 1 (rank 0) the model is the reference's LR (python/LR.py): yhat = b + sum_i w_i.
 *
 * Error codes: FNN_ERR_* of fnn_hip.h; fm_last_error() has the message.
 */
#ifndef FM_HIP_H
#define FM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: what this header declares is what it exports */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef struct fm_handle fm_handle;

const char* fm_last_error(const fm_handle* h);
/* k = rank + 1 (row = [w | v_1..v_rank]), 1 <= k <= 128 (rank 0..127; k >= 17: the wide row layout above);
 * 1 <= n_fields <= 64; 1 <= max_batch <= 4096.  FNN_ERR_ARG otherwise. */
int fm_create(int n_fields, int k, int max_batch, int device, void* stream, fm_handle** out);
int fm_destroy(fm_handle* h);
int fm_sync(fm_handle* h);

/* HOST pointers.  rows [n_rows, k] = concat(W, V) (python/FM.py:19-20); b = the scalar bias (:21). */
int fm_set_table(fm_handle* h, const float* rows, int64_t n_rows);
int fm_get_table(fm_handle* h, float* rows_out);
int fm_get_rows(fm_handle* h, const int64_t* row_ids, int64_t n, float* out);
int fm_set_b(fm_handle* h, float b);
int fm_get_b(fm_handle* h, float* b);

/* One SGD step on a mini-batch.  DEVICE pointers: ids [B, F] int32, y [B] f32; p_out [B] =
 * sigmoid(yhat) before the update (`train_preds`, :42; nullable).  reduce_mean != 0: loss =
 * mean(xent) (the driver's setting), else sum.  loss_out (HOST, nullable; synchronises): the data
 * term of the loss as reduced. */
int fm_train_step(fm_handle* h, const int32_t* ids, const float* y, int B, float lr, float lambda,
                  int reduce_mean, float* p_out, float* loss_out);
/* p_out [B] = sigmoid(yhat) (`test_preds`, :52). */
int fm_predict(fm_handle* h, const int32_t* ids, int B, float* p_out);
/* The same with value weights: wts [B, F] f32, a DEVICE pointer, row-major like ids.  wts == NULL IS the call above: the three
 * entry points without weights forward here with NULL, run the same kernels and give bit-identical results.  fm_eval_w advances
 * wts with ids, max_batch examples a chunk. */
int fm_train_step_w(fm_handle* h, const int32_t* ids, const float* wts, const float* y, int B, float lr, float lambda,
                    int reduce_mean, float* p_out, float* loss_out);
int fm_predict_w(fm_handle* h, const int32_t* ids, const float* wts, int B, float* p_out);

/* The reference's own pre-training schedule (python/ipinyou.py:129-140 and :167-173: batch_size = 1, one step per line).
 * N batch-1 SGD steps in line order, on the handle's stream: example n is trained on the parameters examples 0..n-1 left.
 * DEVICE pointers: ids [N, F] int32 (-1 = absent), wts [N, F] f32 (nullable: every value 1), y [N] f32,
 * p_out [N] (nullable): sigmoid(yhat_n) BEFORE example n's update (`train_preds`).
 * HOST, nullable, either one synchronises: loss_sum_out = sum of the N data losses (accumulated in f64),
 * loss_last_out = example N-1's (the `l` python/ipinyou.py:177 prints).
 * One step is fm_train_step_w at B = 1 (mean and sum coincide): every row of the table takes theta <- theta (1 - lr lambda) - lr g
 * with g at the pre-step values (the dense decay is the lazy scale, advanced once per example), b <- b - lr (delta + lambda b).
 * Right for any ids in [-1, n_rows) whether fm_set_shared_rows is on or off: a row under several columns of one line receives
 * the sum of those columns' contributions in one store, and the result is reproducible bit for bit.  The shared-row marks are
 * not touched: fm_count_shared_rows keeps referring to the last batch step.  An id outside [-1, n_rows) is treated as absent,
 * never dereferenced, and reported by fm_sync as FNN_ERR_RANGE, as fm_train_step does.
 * Every shape fm_create accepts, any N >= 0 (0: nothing happens, FNN_OK), not bounded by max_batch; online calls and batch
 * steps may be interleaved freely.  One persistent workgroup runs the examples of a launch (the work is a dependence chain);
 * a launch takes at most FM_ONLINE_CHUNK examples (environment, read at fm_create; default 65536), and where the call is cut
 * into launches does not change a bit of the result.
 * FNN_ERR_STATE under Adam or FTRL, nothing written: their update is a pass over the whole table per step, per example that is
 * the table's size in traffic, which is not a schedule anybody can run.  FNN_ERR_ARG (before any launch): a null handle, ids or
 * y, N < 0, or lr * lambda outside [0, 1). */
int fm_train_online(fm_handle* h, const int32_t* ids, const float* wts, const float* y, int64_t N,
                    float lr, float lambda, float* p_out, double* loss_sum_out, float* loss_last_out);
/* fm_train_online for several models at once: the reference's driver trains LR and FM on one file (python/ipinyou.py:133, :139),
 * its notebook FM10, FM50 and FM100, each under a learning-rate and L2 search.  Their chains are independent -- one feed, a table
 * each -- so one launch runs them side by side, a workgroup per model, instead of one pass after another on one CU of 256.
 * Model m ends exactly as fm_train_online(hs[m], ids, wts, y, N, lr[m], lambda[m], p_out[m], ..) alone would have left it, bit
 * for bit: table, b, the lazy scale and where it folds, p_out[m], both losses and the range flag (both kernels are the same
 * per-example body).  The models may differ in k (narrow and wide rows mixed), n_rows, lr, lambda, fm_set_shared_rows and the
 * state they start from; they share n_fields and the device.
 * HOST arrays of n_models entries: hs, lr, lambda; p_out (the array or any entry nullable) holds DEVICE pointers [N];
 * loss_sum_out / loss_last_out (nullable; either one synchronises) take every model's losses.  ids, wts (nullable), y: the one
 * DEVICE feed, as in fm_train_online.
 * A launch takes the examples up to the nearest of FM_ONLINE_CHUNK (the smallest among the handles) and the first example whose
 * decay takes ANY model's scale out of [2^-24, 1]; the models that left it are folded before the next launch.  Where the cuts
 * fall changes no bit.  More models than CUs: the surplus workgroups queue; nothing waits on another workgroup.
 * Streams: every launch, fold and copy of the call runs on hs[0]'s stream.  That stream first waits (events) for everything
 * enqueued so far on every other handle's stream, and every other handle's stream then waits for the call's last launch, so
 * the call is ordered after earlier work and before later work on ALL the handles, as if each had run its own fm_train_online.
 * Refused before any launch, nothing written on any model and the loss arrays untouched, the message (with the index of the
 * offending model) in fm_last_error(hs[0]), or fm_last_error(NULL) without a usable hs[0] --
 *   FNN_ERR_ARG: null hs, lr or lambda; a null entry of hs; n_models outside 1..FM_ONLINE_MAX_MODELS; one handle twice (two
 *   workgroups would race on one table); n_fields or device differing from hs[0]'s; N < 0; N > 0 with null ids or y; any
 *   lr[m] * lambda[m] outside [0, 1);
 *   FNN_ERR_STATE: any handle under Adam or FTRL, or without a table.
 * N == 0: FNN_OK, nothing happens.  An id outside [-1, n_rows) is per model (n_rows may differ), absent for that model: a call
 * that synchronises returns FNN_ERR_RANGE and lists the models' indices (their flags are then cleared); otherwise each handle's
 * fm_sync reports its own flag, as after fm_train_online. */
#define FM_ONLINE_MAX_MODELS 1024
int fm_train_online_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const float* y, int64_t N,
                          const float* lr, const float* lambda, float* const* p_out, double* loss_sum_out, float* loss_last_out);
/* fm_train_step_w for several models at once: ONE optimiser step of each of n_models handles on ONE device feed -- the mini-batch
 * schedule of a learning-rate / L2 / rank search, where every model of the search steps on the same lines.  A solo step is four
 * dependent launches and latency-bound, and its first two -- the run sort and the rank merge of the batch's (row, t) keys --
 * depend on the ids only: here the models that agree in n_rows and in the shared-rows mode (a grouping class) share ONE run sort
 * and ONE rank merge, and every other stage is launched once per row layout present (narrow; wide at 16 lanes an example; wide
 * at 32; plain and shared-row forms) with the model as a grid dimension.  One class and one layout under SGD: four launches
 * however many models, plus a fold launch for a model whose lazy scale leaves [2^-24, 1]; Adam / FTRL handles are accepted and
 * keep their dense pass, one launch per model.  n_models == 1 runs the solo step itself (there is nothing to share, and the copy
 * of the argument array would stand in front of it).
 * DEVICE pointers: ids [B, F] int32, wts [B, F] f32 (nullable: every value 1), y [B] f32.  HOST arrays of n_models entries: hs,
 * lr, lambda, reduce_mean (NULL: 0 for every model), p_out (DEVICE pointers [B]; the array or any entry nullable), loss_out
 * (nullable; non-null synchronises).
 * The models may differ in k (1..128, narrow and wide rows mixed), n_rows, optimiser (SGD, Adam, FTRL), the shared-rows mode and
 * the state they start from; they share n_fields and the device.
 * The contract: model m ends exactly as fm_train_step_w(hs[m], ids, wts, y, B, lr[m], lambda[m], reduce_mean[m], p_out[m], &loss)
 * alone would have left it, bit for bit -- the table, b, the lazy SGD scale and the steps at which it folds, the Adam / FTRL
 * state and step count, p_out[m] and loss_out[m], the range flag, and what fm_count_shared_rows(hs[m]) then answers (the same
 * bodies run on the same records).  The one exception is the solo step's own: rows that really sit under several columns of the
 * batch on a shared-rows handle take f32 atomics and are reproducible to rounding only.  Multi steps, solo steps and online
 * calls may be interleaved on the same handles in any order.
 * Streams: everything runs on hs[0]'s stream, which first waits (events) for what is queued on every other handle's stream;
 * every other handle's stream then waits for the call's last launch.
 * Refused before any launch, nothing written on any model and loss_out untouched, the message (with the index of the offending
 * model) in fm_last_error(hs[0]), or fm_last_error(NULL) without a usable hs[0] --
 *   FNN_ERR_ARG: null hs, lr or lambda; a null entry of hs; n_models outside 1..FM_STEP_MAX_MODELS; one handle twice;
 *   n_fields or device differing from hs[0]'s; null ids or y; B < 1 or B above ANY handle's max_batch; any model's lr / lambda
 *   outside what fm_train_step_w accepts for its optimiser (SGD: 0 <= lr * lambda < 1; Adam / FTRL: lr > 0, lambda >= 0);
 *   FNN_ERR_STATE: a handle without a table.
 * An id outside [-1, n_rows) is judged per model (n_rows may differ): absent for that model and never dereferenced.  A call with
 * loss_out returns FNN_ERR_RANGE, lists the models' indices and clears their flags (the losses are still written); without
 * loss_out each handle's fm_sync reports its own flag. */
#define FM_STEP_MAX_MODELS 1024
int fm_train_step_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const float* y, int B,
                        const float* lr, const float* lambda, const int* reduce_mean, float* const* p_out, float* loss_out);
/* which form the handle runs, as fnn_scat1_form() does for its knob: "plain" (the only one built) */
const char* fm_online_form(const fm_handle* h);

/* The optimiser of fm_train_step (python/tf_util.py:15-29); lr and lambda of fm_train_step keep their meaning (base
 * learning rate, L2 weight).  Folds any pending SGD scale into the rows, (re)initialises the state -- Adam: m = v = 0;
 * FTRL: accum = 0.1, linear = 0, the bias's as well -- and resets the step count.  fm_set_table re-initialises the state.
 * beta1 / beta2 / eps: Adam only (TensorFlow's defaults 0.9 / 0.999; eps > 0). */
#define FM_OPT_SGD  0   /* default: the lazy-scale SGD step above */
#define FM_OPT_ADAM 1   /* tf.train.AdamOptimizer(lr, beta1, beta2, eps) */
#define FM_OPT_FTRL 2   /* tf.train.FtrlOptimizer(lr): power -0.5, initial accumulator 0.1, l1 = l2 = 0 */
int fm_set_optimizer(fm_handle* h, int optimizer, float beta1, float beta2, float eps);
/* HOST pointers, each nullable.  s0 / s1 [n_rows, k]: Adam (m, v), FTRL (accum, linear); sb [2]: the bias's; t: steps
 * taken since the state was initialised.  FNN_ERR_STATE under SGD. */
int fm_get_opt_state(fm_handle* h, float* s0, float* s1, float* sb, int64_t* t);
/* Rows shared between columns of a batch (see "Columns and rows" above).  on != 0: the rank merge of every training step marks
 * the rows that sit under more than one column, and the update adds into those with float atomics.  Off by default; legal at any
 * time between steps.  On allocates -- now, or at the next fm_set_table -- and zeroes two int arrays [n_rows] (8 bytes per row);
 * off keeps them for a later on and returns the handle to the launches it ran before. */
int fm_set_shared_rows(fm_handle* h, int on);
/* n_out (HOST): the number of rows the LAST training step found under more than one column -- how ragged the feed is.  A scan
 * of the marks, run on demand and not part of the step; synchronises.  FNN_ERR_STATE while the mode is off, and before the first
 * training step after fm_set_shared_rows turned it on or fm_set_table replaced the table. */
int fm_count_shared_rows(fm_handle* h, int64_t* n_out);
/* DEVICE pointers ids [N, F], y [N] (0 / non-zero).  Predictions in chunks of max_batch, then exact AUC (ties at 1/2),
 * RMSE and logloss (p clipped to [2^-52, 1 - 2^-52]) on the device.  Outputs nullable.  FNN_ERR_RANGE when y holds one
 * class only (auc undefined; rmse and logloss are still written), and when any prediction is NaN or outside [0, 1] (a diverged
 * model; all three outputs are then NaN and fm_last_error gives their number). */
int fm_eval(fm_handle* h, const int32_t* ids, const int32_t* y, int64_t N, double* auc, double* rmse, double* logloss);
int fm_eval_w(fm_handle* h, const int32_t* ids, const float* wts, const int32_t* y, int64_t N,
              double* auc, double* rmse, double* logloss);

/* Predictions and metrics of several models on ONE test feed in one call: what follows fm_train_online_multi in a learning-rate /
 * L2 / rank search, where every model is evaluated on the same lines after every buffer.  One pass of the arguments, one or a few
 * launches per stage for all the models, the library's own radix sort (32-bit keys, a segment per model), one scratch allocation.
 * hs and the outputs auc, rmse, logloss, status: HOST arrays of n_models entries, each output array nullable.  ids [N, F], wts
 * [N, F] (nullable: every value 1), y [N] (0 / non-zero): the one DEVICE feed.  1 <= N <= 2^30, NOT bounded by max_batch.
 * The models may differ in k (narrow and wide rows mixed), n_rows, optimiser (SGD, Adam and FTRL handles all predict) and the
 * shared-rows mode; they share n_fields and the device.  A handle may appear twice: the calls only read it.
 * The contract: p_out[m] (DEVICE, [N]; the entry nullable) is bit for bit what the single-model prediction call writes for
 * hs[m] over the same lines in chunks of max_batch, and auc[m], rmse[m], logloss[m] are bit for bit what the single-model
 * evaluation returns -- the same forward bodies, the same 2,048-example blocks and block-order f64 sums, an integer AUC sum.  A
 * pending lazy SGD scale is applied as those calls apply it; it is not folded and no bit of any model changes.
 * status[m]: FNN_OK, or FNN_ERR_RANGE when model m has a prediction NaN or outside [0, 1] (its three metrics are then NaN).
 * y with one class only: every auc[m] is NaN, rmse and logloss are still written.  An id outside [-1, n_rows) is per model
 * (n_rows may differ) and absent for that model; the evaluation call clears the flags it reports, the prediction call leaves
 * them to each handle's fm_sync.  Any of the three: FNN_ERR_RANGE, the models' indices in fm_last_error(hs[0]).
 * Scratch (evaluation): about 12.5 N bytes per model, in groups of as many models as fit under FM_EVAL_SCRATCH_BYTES
 * (environment, read per call; default 2^30), one model at the least; one allocation per call, and where the groups are cut
 * changes no bit.  The evaluation call synchronises once per group; the prediction call does not synchronise.
 * FM_EVAL_ORDER (environment, read per call): "tile" (default) or "model", the fast index of the prediction grid; same bits.
 * Streams: everything runs on hs[0]'s stream, which first waits (events) for what is queued on every other handle's stream;
 * every other handle's stream then waits for the call's last launch.
 * Refused before any launch, nothing written, the message in fm_last_error(hs[0]) or fm_last_error(NULL) without a usable hs[0] --
 *   FNN_ERR_ARG: null hs or a null entry; n_models outside 1..FM_EVAL_MAX_MODELS; null ids (evaluation: or y; prediction: or
 *   p_out); N outside its range; n_fields or device differing from hs[0]'s;   FNN_ERR_STATE: a handle without a table. */
#define FM_EVAL_MAX_MODELS 1024
int fm_predict_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, int64_t N,
                     float* const* p_out);
int fm_eval_multi(fm_handle* const* hs, int n_models, const int32_t* ids, const float* wts, const int32_t* y,
                  int64_t N, double* auc, double* rmse, double* logloss, int* status);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FM_HIP_H */
