// group_call.h -- a call on a list of handles (fm_api.hip, fnn_api.hip, ipnn_api.hip): what every such call refuses about the
// list itself before any launch, and the streams.
//
// A refusal's message, the entry point's name in front, goes to hs[0], or to the library's own error string without a usable
// hs[0].  Everything a group call launches runs on hs[0]'s stream: enter() has that stream wait for what the other members'
// streams hold so far, leave() -- at the latest the end of the scope, so on every error path too -- has those streams wait for
// it, so that they stay ordered behind what was launched.  Work of a member that enqueues on "the handle's stream" goes through
// on_stream().
//
// H is a family's handle struct: it has F, dev, st, err and the event `join`, used when the handle is hs[0].
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/fnn_hip.h"

namespace fnn {

// runs `fn` with h's launches going to `st` instead of the handle's own stream
template <class H, typename Fn> auto on_stream(H* h, hipStream_t st, Fn fn)
{
    const hipStream_t own = h->st;
    h->st = st;
    auto r = fn();
    h->st = own;
    return r;
}

template <class H> struct GroupCall {
    const char* name;                              // the entry point, in front of every refusal
    H* const* hs; int n, max; H* h0;
    std::string& lib_err;                          // where a refusal goes without a usable hs[0]
    int (*prepare)(H*);                            // nullable: a member's own step in front of the stream join (enter)
    std::vector<hipStream_t> others;               // the streams that are not hs[0]'s, each once
    bool entered = false;
    GroupCall(const char* name_, H* const* hs_, int n_, int max_, std::string& lib_err_, int (*prepare_)(H*) = nullptr)
        : name(name_), hs(hs_), n(n_), max(max_), h0(hs_ && n_ >= 1 && n_ <= max_ ? hs_[0] : nullptr), lib_err(lib_err_), prepare(prepare_) {}
    GroupCall(const GroupCall&) = delete;
    ~GroupCall() { leave(); }
    int refuse(int code, const std::string& msg) const { (h0 ? h0->err : lib_err) = std::string(name) + ": " + msg; return code; }
    static std::string at(const std::string& what, int m) { return "model " + std::to_string(m) + ": " + what; }
    // member h (place m) failed and left the text with itself: hs[0] gets it with the place in front
    int member_failed(int code, const H* h, int m) const { if (h != h0) refuse(code, at(h->err, m)); return code; }
    // The list itself.  twice: why the same handle twice is refused, reported at the later of the two places of the first
    // duplicated pointer; null where it is not refused (reading is not a race), or where the family has a rule of its own.
    int check_list(const char* twice) const
    {
        if (!hs) return refuse(FNN_ERR_ARG, "null hs");
        if (n < 1 || n > max) return refuse(FNN_ERR_ARG, "n_models must be in [1, " + std::to_string(max) + "]");
        for (int m = 0; m < n; ++m) if (!hs[m]) return refuse(FNN_ERR_ARG, at("null handle", m));
        if (twice) {
            std::vector<const H*> seen(hs, hs + n);
            std::sort(seen.begin(), seen.end());
            const auto dup = std::adjacent_find(seen.begin(), seen.end());
            if (dup != seen.end()) {
                int m = n - 1;
                while (hs[m] != *dup) --m;                            // the later of the two places
                return refuse(FNN_ERR_ARG, at(std::string("the same handle twice in one call (") + twice + ")", m));
            }
        }
        for (int m = 1; m < n; ++m)
            if (hs[m]->F != h0->F || hs[m]->dev != h0->dev) return refuse(FNN_ERR_ARG, at("n_fields or device differs from model 0's", m));
        return FNN_OK;
    }
#define GROUP_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { h0->err = std::string(#expr) + ": " + hipGetErrorString(e_); return FNN_ERR_HIP; } } while (0)
    int enter()
    {
        GROUP_HIP(hipSetDevice(h0->dev));
        if (prepare) for (int m = 0; m < n; ++m) {
            const int rc = prepare(hs[m]);
            if (rc != FNN_OK) return member_failed(rc, hs[m], m);
        }
        for (int m = 1; m < n; ++m) if (hs[m]->st != h0->st) others.push_back(hs[m]->st);
        std::sort(others.begin(), others.end());
        others.erase(std::unique(others.begin(), others.end()), others.end());
        if (!others.empty() && !h0->join) GROUP_HIP(hipEventCreateWithFlags(&h0->join, hipEventDisableTiming));
        entered = true;
        for (hipStream_t o : others) {                                // hs[0]'s stream after everything enqueued on the others so far
            GROUP_HIP(hipEventRecord(h0->join, o));
            GROUP_HIP(hipStreamWaitEvent(h0->st, h0->join, 0));
        }
        return FNN_OK;
    }
    int leave()
    {
        if (!entered) return FNN_OK;
        entered = false;
        if (others.empty()) return FNN_OK;                            // whatever the other streams get from here on comes after the call
        GROUP_HIP(hipEventRecord(h0->join, h0->st));
        for (hipStream_t o : others) GROUP_HIP(hipStreamWaitEvent(o, h0->join, 0));
        return FNN_OK;
    }
#undef GROUP_HIP
};

}  // namespace fnn
