// fm_plan.h -- the host arithmetic of the FM calls (fm_api.hip), free of HIP so that a plain C++ program can test it
// (tests/test_host_fm_plan.py): what n_fields and k decide about a handle's kernels (FmPlan, computed once in fm_create), the
// tiles of a batch, when SGD's lazy scale is folded back into the rows, and the order in which a group call lists its members
// for its launches (members_in_class_order).
#pragma once
#include <stdint.h>

namespace fnn {

constexpr int FM_SLOT = 16;                         // floats of a narrow row: SLOT of the FNN path (fm_api.hip asserts it)

// The forward of a handle.  Narrow rows (k <= 16): 16 floats a row, 16 lanes an example.  Wide rows (k >= 17): rup(k, 4) floats a
// row, a lane per float4 piece -- 16 lanes an example while the pieces fit (rw <= 64: rank <= 63), else 32.
enum FmLayout { FM_NARROW = 0, FM_WIDE16 = 1, FM_WIDE32 = 2, FM_LAYOUTS = 3 };
// The sparse-row update of a handle: narrow rows, narrow rows shared between columns (fm_set_shared_rows), wide rows.
enum FmUpdateForm { FM_UPD_NARROW = 0, FM_UPD_SHARED = 1, FM_UPD_WIDE = 2, FM_UPDATE_FORMS = 3 };

struct FmPlan {
    int F = 0, K = 0;                               // n_fields, k (= rank + 1)
    bool wide = false;                              // k >= 17
    int rw = FM_SLOT;                               // row stride in floats
    int K1p = 0;                                    // gx' of an example in floats: a slot per field of rup(F, 16), or [F][rw]
    int layout = FM_NARROW;                         // FmLayout
    int nf = 1;                                     // fields per lane (narrow) = chunks of 16 fields (wide): ceil(F / 16), 1..4
    int epb = 16;                                   // examples per workgroup of 256 lanes: 16, or 8 at 32 lanes an example
    int form = FM_UPD_NARROW;                       // FmUpdateForm; the one entry that fm_set_shared_rows changes (fm_update_form)
};

inline int fm_update_form(const FmPlan& p, bool shared) { return p.wide ? FM_UPD_WIDE : shared ? FM_UPD_SHARED : FM_UPD_NARROW; }

// 1 <= F <= 64, 1 <= k <= 128 (fm_create refuses anything else)
inline FmPlan fm_make_plan(int F, int k, bool shared = false)
{
    FmPlan p;
    p.F = F; p.K = k;
    p.wide = k > FM_SLOT;
    p.rw = p.wide ? (k + 3) / 4 * 4 : FM_SLOT;
    p.nf = (F + 15) / 16;
    p.K1p = p.wide ? F * p.rw : p.nf * 16 * FM_SLOT;
    p.layout = !p.wide ? FM_NARROW : p.rw <= 64 ? FM_WIDE16 : FM_WIDE32;
    p.epb = p.layout == FM_WIDE32 ? 8 : 16;
    p.form = fm_update_form(p, shared);
    return p;
}

// the forward's workgroups over B examples at epb examples each
inline int64_t fm_tiles(int64_t B, int epb) { return (B + epb - 1) / epb; }

// SGD's dense L2 decay is kept as a lazy scale beside the rows; it is folded into them once it leaves [2^-24, 1]
inline bool fm_fold_due(double scale) { return scale < 5.96e-8 || scale > 1.0; }

// A group call launches once per class present (layout class or update form: NC = 3 classes), its members listed class by class,
// list order inside a class: cnt[c] members of class c from place first[c] on.  place(j, m): member m stands at place j.
template <int NC> struct ClassRuns { int cnt[NC], first[NC]; };
template <int NC, class ClassOf, class Place> ClassRuns<NC> members_in_class_order(int n, ClassOf class_of, Place place)
{
    ClassRuns<NC> r;
    int pos[NC];
    for (int c = 0; c < NC; ++c) r.cnt[c] = 0;
    for (int m = 0; m < n; ++m) ++r.cnt[class_of(m)];
    for (int c = 0; c < NC; ++c) pos[c] = r.first[c] = c ? r.first[c - 1] + r.cnt[c - 1] : 0;
    for (int m = 0; m < n; ++m) place(pos[class_of(m)]++, m);
    return r;
}

}  // namespace fnn
