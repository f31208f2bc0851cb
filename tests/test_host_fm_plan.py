"""The host arithmetic of the FM calls (deep-ctr_amd/csrc/fm_plan.h, free of HIP): what n_fields and k decide about a handle's
kernels (FmPlan), the tiles of a batch, when the lazy scale folds, and the order in which a group call lists its members for its
launches.  A stand-alone C++ program with its own main, built with the address and undefined-behaviour sanitizers, prints them;
nothing is loaded into Python.  What it prints is compared with a restatement written from include/fm_hip.h ("Row layout on the
device": k <= 16 keeps 16-float rows, a lane per field up to 16 fields, beyond that lane f takes fields f, f + 16, ..; k >= 17
takes rows of rup(k, 4) floats, every row piece one 16-byte access, a quarter or half wave per example, 16 fields at a time) and
from DESIGN.md ("The FM calls' host side"), not from the header under test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = range(1, 65)
KS = (1, 16, 17, 64, 65, 128)
BATCHES = (1, 7, 8, 9, 16, 17, 33, 4096, 100000)
SCALES = (1.0, 1.0000001, 0.5, 6.0e-8, 5.9e-8, 2.0 ** -23, 2.0 ** -25, 0.0, 2.0)
# hand-made member lists, a class (0..2) per member: all of one class, every class present, a class absent in the middle, a
# single member, and a list that is already in class order / in reverse order
LISTS = ([0, 0, 0, 0], [1, 1, 1], [2, 2], [2, 0, 1, 0, 2, 1, 1], [2, 0, 2, 0, 0], [0], [1], [2], [0, 1, 2], [2, 1, 0], [1, 2, 1, 2])

PROGRAM = r"""
#include "fm_plan.h"

#include <cstdio>
#include <vector>

using namespace fnn;

int main()
{
    const int ks[] = {%(ks)s};
    for (int F = 1; F <= 64; ++F)
        for (int k : ks) {
            const FmPlan p = fm_make_plan(F, k), s = fm_make_plan(F, k, true);
            std::printf("plan %%d %%d : %%d %%d %%d %%d %%d %%d %%d %%d\n", p.F, p.K, (int)p.wide, p.rw, p.K1p, p.layout, p.nf, p.epb, p.form, s.form);
            // the shared-rows mode changes the update form and nothing else
            FmPlan q = p;
            q.form = fm_update_form(q, true);
            if (q.form != s.form || s.wide != p.wide || s.rw != p.rw || s.K1p != p.K1p || s.layout != p.layout || s.nf != p.nf || s.epb != p.epb) return 2;
        }
    const long long bs[] = {%(bs)s};
    for (long long B : bs) std::printf("tiles %%lld : %%lld %%lld\n", B, (long long)fm_tiles(B, 16), (long long)fm_tiles(B, 8));
    const double scales[] = {%(scales)s};
    for (double s : scales) std::printf("fold %%.17g : %%d\n", s, (int)fm_fold_due(s));
    const std::vector<std::vector<int>> lists = {%(lists)s};
    for (const std::vector<int>& cls : lists) {
        std::vector<int> at(cls.size(), -1);
        int calls = 0;
        const ClassRuns<3> r = members_in_class_order<3>((int)cls.size(), [&](int m) { return cls[m]; },
                                                         [&](int j, int m) { at[j] = m; ++calls; });
        if (calls != (int)cls.size()) return 3;
        std::printf("order cnt %%d %%d %%d first %%d %%d %%d members", r.cnt[0], r.cnt[1], r.cnt[2], r.first[0], r.first[1], r.first[2]);
        for (int m : at) std::printf(" %%d", m);
        std::printf("\n");
    }
    std::puts("fm_plan OK");
    return 0;
}
"""


def plan(F, k, shared):
    """(wide, rw, K1p, layout, fields per lane, examples per workgroup, update form) as the documents state them."""
    wide = k >= 17
    rw = -(-k // 4) * 4 if wide else 16                   # floats a row: 64 bytes, or rup(k, 4)
    pieces = rw // 4                                      # 16-byte pieces of a row: a lane each on the wide path
    lanes = 32 if wide and pieces > 16 else 16            # a quarter wave while the pieces fit it, else a half
    layout = 0 if not wide else 1 if lanes == 16 else 2   # narrow; wide at 16 lanes an example; wide at 32
    groups = -(-F // 16)                                  # 16 fields at a time: fields per lane / chunks of 16
    K1p = F * rw if wide else groups * 16 * 16            # gx' of an example: [F][rw], or a 16-float slot per field of rup(F, 16)
    form = 2 if wide else 1 if shared else 0              # narrow, narrow shared, wide
    return int(wide), rw, K1p, layout, groups, 256 // lanes, form


def expected():
    out = []
    for F in FIELDS:
        for k in KS:
            p = plan(F, k, False)
            out.append("plan %d %d : %d %d %d %d %d %d %d %d" % ((F, k) + p + (plan(F, k, True)[-1],)))
    for B in BATCHES:
        out.append("tiles %d : %d %d" % (B, -(-B // 16), -(-B // 8)))
    for s in SCALES:
        out.append("fold %.17g : %d" % (s, int(not (5.96e-8 <= s <= 1.0))))       # outside [2^-24, 1], the bound written 5.96e-8
    for cls in LISTS:
        cnt = [cls.count(c) for c in range(3)]
        members = sorted(range(len(cls)), key=lambda m: cls[m])                  # stable: list order inside a class
        out.append("order cnt %d %d %d first %d %d %d members %s" % (tuple(cnt) + (0, cnt[0], cnt[0] + cnt[1]) + (' '.join(map(str, members)),)))
    out.append("fm_plan OK")
    return out


def test_restatement_covers_the_documented_limits():
    """The restatement itself at the shapes the documents name: k = 101 gives rows of 104 floats (fm_hip.h), rank 63 is the last at
    16 lanes an example and 39 fields are three groups of 16."""
    assert plan(16, 101, False)[:2] == (1, 104)
    assert plan(16, 64, False)[3] == 1 and plan(16, 65, False)[3] == 2 and plan(16, 16, False)[3] == 0
    assert plan(39, 11, False)[4] == 3 and plan(39, 11, False)[2] == 48 * 16 and plan(39, 51, False)[2] == 39 * 52
    assert plan(16, 65, False)[5] == 8 and plan(16, 64, False)[5] == 16


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ on this machine")
def test_plans_tiles_fold_and_class_order_under_the_sanitizers(tmp_path):
    src = tmp_path / "fm_plan_test.cpp"
    exe = tmp_path / "fm_plan_test"
    src.write_text(PROGRAM % {'ks': ', '.join(map(str, KS)), 'bs': ', '.join('%dll' % b for b in BATCHES),
                              'scales': ', '.join('%.17g' % s for s in SCALES),
                              'lists': ', '.join('{%s}' % ', '.join(map(str, l)) for l in LISTS)})
    # (the sanitizers' runtimes linked into the program: it then starts whatever else the environment has the loader bring in)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "deep-ctr_amd", "csrc"), str(src), "-o", str(exe)], check=True, cwd=ROOT)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    got, want = run.stdout.splitlines(), expected()
    assert len(got) == len(want) == 64 * len(KS) + len(BATCHES) + len(SCALES) + len(LISTS) + 1
    for g, w in zip(got, want):
        assert g == w
