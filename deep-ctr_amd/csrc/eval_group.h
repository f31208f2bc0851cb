// eval_group.h -- the host arithmetic of the calls that evaluate many models on one feed (fm_eval_multi, fnn_eval_multi,
// ipnn_eval_multi), free of HIP so that a plain C++ program can test it (tests/test_host_eval_group.py): how many models share
// one scratch allocation, what a model's sums become, and the call's final message.  The loop that uses them is eval_groups()
// (metrics.hip.h).  Also what every group call, the step calls included, does with its list of members on the host: their
// launch classes (class_index) and the model list of a refusal (eval_list_add).
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <string>

#include "../../include/fnn_hip.h"

namespace fnn {

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// What metrics_multi leaves per model (metrics.hip.h): the sums of the squared errors and of the log losses, the AUC's integer
// sum (auc = auc_sum / (2 n_pos n_neg)), and the number of predictions NaN or outside [0, 1].
struct MetricOut { double se, ll; unsigned long long auc_sum, n_bad; };

// The scratch cap of one group of models: $env when it holds a number >= 1 (read per call), else 2^30 bytes.
inline size_t eval_scratch_cap(const char* env)
{
    size_t cap = (size_t)1 << 30;
    if (const char* e = getenv(env)) { const long long c = atoll(e); if (c >= 1) cap = (size_t)c; }
    return cap;
}

// The models of a group share one scratch allocation of bytes(g): as many of the n as fit under the cap, one at the least.
template <typename Bytes> int eval_group_size(int n, size_t cap, Bytes bytes)
{
    int G = n;
    const size_t one = bytes(1);
    if ((size_t)G > cap / one) G = (int)(cap / one);
    if (G < 1) G = 1;
    while (G > 1 && bytes(G) > cap) --G;
    return G;
}

// A model's metrics from its sums over the N lines, n_pos of them positive: bit for bit device_metrics' values.  Any bad
// prediction: all three NaN and status FNN_ERR_RANGE (roc_auc_score and log_loss raise ValueError on such input); one class
// only: auc NaN, the other two written.
struct EvalValues { double auc, rmse, logloss; int status; };
inline EvalValues eval_values(const MetricOut& o, unsigned long long n_pos, int64_t N)
{
    const double nan = std::nan("");
    if (o.n_bad) return EvalValues{nan, nan, nan, FNN_ERR_RANGE};
    const bool two = n_pos > 0 && (int64_t)n_pos < N;
    const double np_ = (double)n_pos, nn = (double)(N - (int64_t)n_pos);
    return EvalValues{two ? (double)o.auc_sum / (2.0 * np_ * nn) : nan, std::sqrt(o.se / (double)N), o.ll / (double)N, FNN_OK};
}

// "0, 3, 7": the list of models inside a clause of the verdict
inline void eval_list_add(std::string& list, int model) { list += (list.empty() ? "" : ", ") + std::to_string(model); }

// The class of `c` among `classes`: the index of the first one that same(classes[i], c) accepts, `c` appended when none does --
// so classes stand in the order of their first members.
template <class V, class T, class Same> size_t class_index(V& classes, const T& c, Same same)
{
    size_t i = 0;
    while (i < classes.size() && !same(classes[i], c)) ++i;
    if (i == classes.size()) classes.push_back(c);
    return i;
}
// (classes that compare themselves: a.same(b))
template <class V, class T> size_t class_index(V& classes, const T& c)
{
    return class_index(classes, c, [](const T& a, const T& b) { return a.same(b); });
}

// The message of an evaluation that returns FNN_ERR_RANGE, empty when nothing is wrong: up to three clauses joined by "; " --
// the models (`bad`, a list as above) with predictions NaN or outside [0, 1], the models (`range`) that met a feature id outside
// `id_range` ("[-1, n_rows)" for FM and FNN, "[0, n_rows)" for the inner-product family), and a feed of one class.
inline std::string eval_verdict(const std::string& bad, const std::string& range, bool one_class, const char* id_range)
{
    std::string msg;
    auto clause = [&](const std::string& c) { msg += (msg.empty() ? "" : "; ") + c; };
    if (!bad.empty()) clause("predictions NaN or outside [0, 1] in model(s) " + bad);
    if (!range.empty()) clause(std::string("feature id outside ") + id_range + " in model(s) " + range);
    if (one_class) clause("only one class present in y (roc_auc_score raises ValueError)");
    return msg;
}
inline std::string eval_verdict(const std::string& bad, const std::string& range, unsigned long long n_pos, int64_t N, const char* id_range)
{
    return eval_verdict(bad, range, n_pos == 0 || (int64_t)n_pos == N, id_range);
}

}  // namespace fnn
