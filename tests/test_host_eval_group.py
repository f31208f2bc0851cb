"""The host arithmetic of fm_eval_multi / fnn_eval_multi / ipnn_eval_multi (deep-ctr_amd/csrc/eval_group.h, free of HIP): the
group size under the scratch cap, a model's metrics from its sums, the call's final message, and the launch classes of a list of
members (class_index, which the step calls use too).  A stand-alone C++ program with its own main, built with the address and
undefined-behaviour sanitizers and run; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include "eval_group.h"

#include <cstdio>
#include <limits>
#include <vector>

using namespace fnn;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static void group_size()
{
    // a linear bytes(g): as many as fit, one at the least, never more than there are
    for (size_t one : {(size_t)1, (size_t)256, (size_t)1000, (size_t)4097})
        for (size_t cap : {(size_t)1, (size_t)255, (size_t)256, (size_t)999, (size_t)1000, (size_t)1001, (size_t)65536, (size_t)1 << 30})
            for (int n : {1, 2, 3, 16, 1024}) {
                auto bytes = [one](int g) { return (size_t)g * one; };
                const int G = eval_group_size(n, cap, bytes);
                const size_t fit = cap / one < 1 ? 1 : cap / one;
                CHECK(G >= 1 && G <= n);
                CHECK(G == 1 || bytes(G) <= cap);
                CHECK((size_t)G == ((size_t)n < fit ? (size_t)n : fit));
                if (cap < one) CHECK(G == 1);
            }
    // bytes(g) rounded up in pieces, as the scratch of a group is, with a constant piece: g * bytes(1) overestimates and
    // underestimates by turns, and the result still fits
    for (size_t line : {(size_t)4, (size_t)100, (size_t)4000})
        for (size_t cap : {(size_t)1, (size_t)512, (size_t)5000, (size_t)100000, (size_t)1 << 20})
            for (int n : {1, 2, 7, 64}) {
                auto bytes = [line](int g) { return up256((size_t)g * line) + up256((size_t)g * 32) + up256((size_t)g * 4) + 256; };
                const int G = eval_group_size(n, cap, bytes);
                CHECK(G >= 1 && G <= n);
                CHECK(G == 1 || bytes(G) <= cap);
                if (cap < bytes(1)) CHECK(G == 1);
                if (G < n && G > 1) CHECK(bytes(G + 1) > cap || (size_t)(G + 1) > cap / bytes(1));
            }
    CHECK(up256(0) == 0 && up256(1) == 256 && up256(256) == 256 && up256(257) == 512);
}

static void verdict()
{
    const char* fm = "[-1, n_rows)";
    const char* ip = "[0, n_rows)";
    const std::string bad = "predictions NaN or outside [0, 1] in model(s) 1";
    const std::string range = "feature id outside [-1, n_rows) in model(s) 1";
    const std::string one = "only one class present in y (roc_auc_score raises ValueError)";
    CHECK(eval_verdict("", "", 3ull, 10, fm).empty());
    CHECK(eval_verdict("", "", false, ip).empty());
    // each clause alone: with the entry point's name in front, the strings the GPU tests compare with ==
    CHECK("fnn_eval_multi: " + eval_verdict("1", "", 3ull, 10, fm) == "fnn_eval_multi: predictions NaN or outside [0, 1] in model(s) 1");
    CHECK("fnn_eval_multi: " + eval_verdict("", "", 0ull, 10, fm) == "fnn_eval_multi: only one class present in y (roc_auc_score raises ValueError)");
    CHECK("fnn_eval_multi: " + eval_verdict("", "", 10ull, 10, fm) == "fnn_eval_multi: only one class present in y (roc_auc_score raises ValueError)");
    CHECK("fnn_eval_multi: " + eval_verdict("", "1", 3ull, 10, fm) == "fnn_eval_multi: feature id outside [-1, n_rows) in model(s) 1");
    CHECK("ipnn_eval_multi: " + eval_verdict("", "0", false, ip) == "ipnn_eval_multi: feature id outside [0, n_rows) in model(s) 0");
    CHECK("ipnn_eval_multi: " + eval_verdict("0", "", 3ull, 10, ip) == "ipnn_eval_multi: predictions NaN or outside [0, 1] in model(s) 0");
    // two and three: "; " between them, in the order bad, range, one class
    CHECK(eval_verdict("1", "1", 3ull, 10, fm) == bad + "; " + range);
    CHECK(eval_verdict("1", "", 0ull, 10, fm) == bad + "; " + one);
    CHECK(eval_verdict("", "1", 10ull, 10, fm) == range + "; " + one);
    CHECK(eval_verdict("1", "1", 0ull, 10, fm) == bad + "; " + range + "; " + one);
    CHECK(eval_verdict("1", "1", true, fm) == bad + "; " + range + "; " + one);
    // the lists
    std::string l;
    eval_list_add(l, 0); CHECK(l == "0");
    eval_list_add(l, 3); eval_list_add(l, 1023); CHECK(l == "0, 3, 1023");
}

static void values()
{
    const int64_t N = 8;
    // two classes, nothing bad: auc_sum / (2 n_pos n_neg), sqrt(se / N), ll / N
    EvalValues v = eval_values(MetricOut{2.0, 4.0, 15ull, 0ull}, 3ull, N);
    CHECK(v.auc == 15.0 / (2.0 * 3.0 * 5.0) && v.rmse == std::sqrt(2.0 / 8.0) && v.logloss == 4.0 / 8.0 && v.status == FNN_OK);
    // any bad prediction: three NaNs and FNN_ERR_RANGE, whatever the sums hold
    v = eval_values(MetricOut{2.0, 4.0, 15ull, 1ull}, 3ull, N);
    CHECK(std::isnan(v.auc) && std::isnan(v.rmse) && std::isnan(v.logloss) && v.status == FNN_ERR_RANGE);
    v = eval_values(MetricOut{2.0, 4.0, 0ull, std::numeric_limits<unsigned long long>::max()}, 0ull, N);
    CHECK(std::isnan(v.auc) && std::isnan(v.rmse) && std::isnan(v.logloss) && v.status == FNN_ERR_RANGE);
    // one class only (no positives; nothing but positives): auc NaN, the other two finite, the model itself is fine
    for (unsigned long long n_pos : {0ull, 8ull}) {
        v = eval_values(MetricOut{2.0, 4.0, 0ull, 0ull}, n_pos, N);
        CHECK(std::isnan(v.auc) && std::isfinite(v.rmse) && std::isfinite(v.logloss) && v.status == FNN_OK);
        CHECK(v.rmse == 0.5 && v.logloss == 0.5);
    }
}

static void cap()
{
    unsetenv("EVAL_GROUP_TEST_CAP");
    CHECK(eval_scratch_cap("EVAL_GROUP_TEST_CAP") == (size_t)1 << 30);
    setenv("EVAL_GROUP_TEST_CAP", "12345", 1);
    CHECK(eval_scratch_cap("EVAL_GROUP_TEST_CAP") == 12345);
    setenv("EVAL_GROUP_TEST_CAP", "0", 1);
    CHECK(eval_scratch_cap("EVAL_GROUP_TEST_CAP") == (size_t)1 << 30);
    setenv("EVAL_GROUP_TEST_CAP", "nonsense", 1);
    CHECK(eval_scratch_cap("EVAL_GROUP_TEST_CAP") == (size_t)1 << 30);
}

// A launch class as the group calls have them: what is compared (key) and what is not (tag: who opened the class).
struct Cls {
    int key, tag;
    bool same(const Cls& o) const { return key == o.key; }
};

static void classes()
{
    auto eq = [](const Cls& a, const Cls& b) { return a.key == b.key; };
    // an empty list: the element opens class 0
    std::vector<Cls> v;
    CHECK(class_index(v, Cls{5, 0}, eq) == 0 && v.size() == 1 && v[0].key == 5 && v[0].tag == 0);
    // every element new: one class each, in the order they came
    v.clear();
    for (int m = 0; m < 7; ++m) CHECK(class_index(v, Cls{10 * m, m}, eq) == (size_t)m);
    CHECK(v.size() == 7);
    for (int m = 0; m < 7; ++m) CHECK(v[m].key == 10 * m && v[m].tag == m);
    // every element equal: class 0, which stays its first member's
    v.clear();
    for (int m = 0; m < 7; ++m) CHECK(class_index(v, Cls{4, m}, eq) == 0);
    CHECK(v.size() == 1 && v[0].tag == 0);
    // an element that equals only a later class gets that class's index, not a new one; nothing in front of it moves
    v = {Cls{1, 0}, Cls{2, 1}, Cls{3, 2}};
    CHECK(class_index(v, Cls{3, 9}, eq) == 2 && v.size() == 3);
    CHECK(class_index(v, Cls{2, 9}, eq) == 1 && v.size() == 3);
    CHECK(class_index(v, Cls{4, 3}, eq) == 3 && v.size() == 4);
    for (int m = 0; m < 4; ++m) CHECK(v[m].key == m + 1 && v[m].tag == m);
    // a predicate that accepts several classes: always the FIRST of them
    auto parity = [](const Cls& a, const Cls& b) { return (a.key & 1) == (b.key & 1); };
    v = {Cls{2, 0}, Cls{3, 1}, Cls{5, 2}, Cls{4, 3}};
    CHECK(class_index(v, Cls{7, 9}, parity) == 1);
    CHECK(class_index(v, Cls{8, 9}, parity) == 0);
    CHECK(v.size() == 4);
    for (int m = 0; m < 4; ++m) CHECK(v[m].tag == m);
    // the form without a predicate is same() of the classes themselves
    v.clear();
    const int keys[] = {6, 8, 6, 7, 8, 6};
    const size_t want[] = {0, 1, 0, 2, 1, 0};
    for (int m = 0; m < 6; ++m) CHECK(class_index(v, Cls{keys[m], m}) == want[m]);
    CHECK(v.size() == 3 && v[0].tag == 0 && v[1].tag == 1 && v[2].tag == 3);
    // members appended through the index, as the calls do: first-member order of the classes, list order inside each
    struct WithMembers { int key; std::vector<int> members; };
    std::vector<WithMembers> w;
    for (int m = 0; m < 6; ++m)
        w[class_index(w, WithMembers{keys[m], {}}, [](const WithMembers& a, const WithMembers& b) { return a.key == b.key; })].members.push_back(m);
    CHECK(w.size() == 3 && w[0].members == (std::vector<int>{0, 2, 5}) && w[1].members == (std::vector<int>{1, 4}) && w[2].members == (std::vector<int>{3}));
}

int main()
{
    group_size();
    verdict();
    values();
    cap();
    classes();
    if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    std::puts("eval_group OK");
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ on this machine")
def test_group_size_values_and_verdict_under_the_sanitizers(tmp_path):
    src = tmp_path / "eval_group_test.cpp"
    exe = tmp_path / "eval_group_test"
    src.write_text(PROGRAM)
    # (the sanitizers' runtimes linked into the program: it then starts whatever else the environment has the loader bring in)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "deep-ctr_amd", "csrc"), str(src), "-o", str(exe)], check=True, cwd=ROOT)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "eval_group OK"
