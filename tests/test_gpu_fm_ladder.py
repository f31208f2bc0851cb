"""Every rung of the FM calls' dispatch ladder (fm_ladder in deep-ctr_amd/csrc/fm_api.hip: fields per lane 1..4 x value weights
or none x layout class -- narrow rows, wide rows at 16 lanes an example, wide at 32 -- and the width of the sort keys where a rank
merge rides beside the forward) at the smallest shapes that reach it, on the device.

The group calls are held to solo twins BIT FOR BIT (check_group of test_gpu_fm_step_multi.py: every step's p and loss, then
table and b), with every row under one column: F in {16, 17, 33, 49} gives 1..4 fields per lane, the members' k of 11, 17 and 65
the three layout classes in one group, B = 33 is no multiple of 16 or 8, and two consecutive steps read what the first wrote.
After the steps predict_many on the group against each member's own forward, as bits.  Eight cases: the 24 instances of the
evaluation group and the 24 of launch 2 of the step group with 32-bit keys; one more case has the 64-bit keys.

Group against solo cannot see a rung mis-picked for both.  The solo forwards are held to the float64 restatements by
test_gpu_fm_fields.py, test_gpu_fm_wide.py and test_gpu_fm_weights.py ("The FM calls' host side", lists which reaches
which); the two solo instances none of them reaches -- value weights on wide rows at 16 lanes with 49..64 fields, and at 32 lanes
with 17..32 fields -- are held here to tests/fm_weighted_ref.py by test_gpu_fm_weights.sgd_vs_oracle_w, at its bounds unchanged."""
import numpy as np
import pytest

import fm_shared_cases as sc
from test_gpu_fm_fields import model, table
from test_gpu_fm_step_multi import BIG, PER, Spec, bits, check_group, zipf_steps
from test_gpu_fm_weights import sgd_vs_oracle_w, wbatches

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import synth
from deep_ctr_amd.FM import predict_many, train_step_many

pytestmark = pytest.mark.gpu
B = 33


def members(F, n_rows=None, ks=(11, 17, 65)):
    return [Spec(F, k, lr=0.03 + 0.01 * i, lam=(1e-2, 0.0, 2e-2)[i % 3], seed=60 + i, n_rows=n_rows, mean=i % 2) for i, k in enumerate(ks)]


def predictions_equal_the_members_own(specs, steps):
    """The group trained by train_step_many, then predict_many on it against every member's own forward, as bits."""
    models = [s.model(B) for s in specs]
    try:
        for ids, wts, y in steps:
            train_step_many(models, ids, y, wts=wts)
        ids, wts, _ = steps[-1]
        many = predict_many(models, ids, wts=wts)
        for i, (m, p) in enumerate(zip(models, many)):
            own = m.forward(ids, wts=wts).cpu().numpy()
            assert np.isfinite(own).all() and own.std() > 0, i
            assert np.array_equal(bits(p.cpu().numpy()), bits(own)), 'model %d (F %d k %d)' % (i, specs[i].F, specs[i].k)
    finally:
        for m in models:
            m.close()


@pytest.mark.parametrize("weighted", [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize("F", [16, 17, 33, 49])
def test_every_layout_class_at_every_field_group_count(built, F, weighted):
    specs = members(F)
    assert specs[0].n_rows == sc.n_rows_of(F, PER) < 1000
    steps = zipf_steps(F, B, 2, 900 + F, weighted)
    got = check_group(specs, steps)
    for s, r in zip(specs, got):
        assert not np.array_equal(r['state'][0], s.rows().astype(np.float32))               # every member was trained
    predictions_equal_the_members_own(specs, steps)


def test_64_bit_keys_on_narrow_and_wide_rows(built):
    """17 fields (two per lane), no weights, k = 4 and k = 17 on the 1,100,000-row table, whose keys (row * 4096 + example) need
    64 bits; the ids moved to the top of the table, so that the keys' high halves are in use."""
    F = 17
    assert BIG * 4096 > 2 ** 32
    steps = []
    for ids, wts, y in zipf_steps(F, B, 2, 950, False):
        steps.append((np.where(ids >= sc.S_ROWS, ids + (BIG - sc.n_rows_of(F, PER)), ids).astype(np.int32), wts, y))
    assert max(int(s[0].max()) for s in steps) * 4096 > 2 ** 32
    specs = members(F, n_rows=BIG, ks=(4, 17))
    check_group(specs, steps)
    predictions_equal_the_members_own(specs, steps)


@pytest.mark.parametrize("F,rank", [(49, 16), (64, 63), (17, 64), (32, 127)], ids=['L16-NC4-F49', 'L16-NC4-F64', 'L32-NC2-F17', 'L32-NC2-F32'])
def test_weighted_solo_forwards_no_other_file_reaches(built, F, rank):
    """The forward and the first SGD step (p, loss, the updated rows and b) of the weighted wide kernels at 16 lanes with four
    chunks of fields and at 32 lanes with two, each at the first and last rank and field count of its rung; B = 9: a partial
    workgroup at 16 examples a workgroup, a full and a partial one at 8."""
    sizes = synth.field_sizes_tiny(500, F)
    rows = table(sum(sizes) + 24, F, rank, 3 + F)
    m = model(F, rank, 9, ['sgd', 0.05, 'sum'], 1e-2, rows, 0.1)
    try:
        sgd_vs_oracle_w(m, rows, 0.1, wbatches(sizes, 9, 1, 300 + F, gap=24), 0.05, 1e-2, 0)
    finally:
        m.close()
