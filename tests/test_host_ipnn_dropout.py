"""Drawn keep-masks of the inner-product family on the host side: the NumPy restatement of the draw (deep_ctr_amd.dropout:
Philox4x32-10's known answers, the prefix property, the independence of seed / step / layer, the keep rate), the `Drawn` value
type, and the two entry points -- declared in include/ipnn_hip.h, bound in _capi, exported by the built library, ipnn_cfg
untouched.

Statistical bounds are those of fair coin flips: a rate over n elements has sigma = sqrt(p (1 - p) / n); the seed and step are
fixed, so every figure below is one number, not a distribution (the restatement's own values are in the comments)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deep_ctr_amd  # noqa: F401
from deep_ctr_amd import _capi, dropout
from deep_ctr_amd.ipnn import Drawn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ipnn_train_step_drawn", "ipnn_draw_masks")

# (counter, key, output): Random123's known-answer vectors for philox4x32-10
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT, ids=['zeros', 'ones', 'pi'])
def test_philox_known_answers(counter, key, want):
    got = dropout.philox4x32_10(counter, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert tuple(int(v) for v in got) == want


def test_philox_broadcasts_like_its_scalar_calls():
    c0 = np.arange(5, dtype=np.uint64)[:, None]
    c1 = np.array([0, 7, 1 << 16], dtype=np.uint64)[None, :]
    got = dropout.philox4x32_10((c0, c1, 3, 0xffffffff), (1234, 0))
    assert got.shape == (5, 3, 4)
    for i in range(5):
        for j in range(3):
            assert np.array_equal(got[i, j], dropout.philox4x32_10((int(c0[i, 0]), int(c1[0, j]), 3, 0xffffffff), (1234, 0)))


def test_masks_follow_the_counter_layout():
    """One element by hand: layer 2, example 9 (group 2, word 1), column 5, of step 2^32 + 7 under seed 2^40 + 3."""
    seed, step = (1 << 40) + 3, (1 << 32) + 7
    w = dropout.philox4x32_10((5, (2 << 16) | (9 >> 2), 7, 1), (3, 1 << 8))
    m = dropout.drawn_masks(seed, step, 10, (3, 4, 6), 0.5)
    assert [x.shape for x in m] == [(10, 3), (10, 4), (10, 6)] and all(x.dtype == np.uint8 for x in m)
    assert m[2][9, 5] == (1 if int(w[1]) < (1 << 31) else 0)
    assert dropout.threshold(0.5) == 1 << 31 and dropout.threshold(1.0) is None
    assert dropout.threshold(0.7) == int(np.floor(float(np.float32(0.7)) * 4294967296.0))      # the float32 of ipnn_cfg, not the double


def test_prefix_property():
    """The mask of an element depends on neither B nor d."""
    big = dropout.drawn_masks(1234, 7, 4096, (297, 1000, 64), 0.5)
    small = dropout.drawn_masks(1234, 7, 17, (100, 1000, 30), 0.5)
    for t in range(3):
        assert np.array_equal(small[t], big[t][:17, :small[t].shape[1]])
    one = dropout.drawn_masks(1234, 7, 1, (297,), 0.5)
    assert np.array_equal(one[0], big[0][:1])


def test_seed_step_and_layer_each_change_the_mask():
    """257 x 297 coin flips agree with an independent set in half of the places: sigma = 0.5 / sqrt(257 * 297) = 0.0018, bound
    4 sigma.  (The restatement: 0.502 / 0.498 / 0.500 for step + 1 / seed + 1 / layer + 1.)"""
    B, d, seed, step = 257, 297, 1234, 7
    base = dropout.drawn_masks(seed, step, B, (d, d), 0.5)
    others = {
        'step+1': dropout.drawn_masks(seed, step + 1, B, (d,), 0.5)[0],
        'seed+1': dropout.drawn_masks(seed + 1, step, B, (d,), 0.5)[0],
        'layer+1': base[1],
        'step+2^32': dropout.drawn_masks(seed, step + (1 << 32), B, (d,), 0.5)[0],
        'seed+2^32': dropout.drawn_masks(seed + (1 << 32), step, B, (d,), 0.5)[0],
    }
    sigma = 0.5 / np.sqrt(B * d)
    for name, m in others.items():
        agree = float((m == base[0]).mean())
        print("[dropout] %s agrees with the original in %.4f of the places" % (name, agree))
        assert not np.array_equal(m, base[0]), name
        assert abs(agree - 0.5) <= 4 * sigma, (name, agree)


@pytest.fixture(scope="module")
def rate_masks():
    return {kp: dropout.drawn_masks(1234, 7, 4096, (297, 1000, 64), kp) for kp in (0.5, 0.7)}


@pytest.mark.parametrize("kp", [0.5, 0.7])
def test_keep_rate(rate_masks, kp):
    """Overall rate of every layer within 4 sigma of keep_prob, every row's and every column's within 5 sigma (the restatement:
    below 2 sigma overall, 4.0 sigma at worst over all rows and columns)."""
    p = float(np.float32(kp))
    for t, m in enumerate(rate_masks[kp]):
        B, d = m.shape
        z = abs(float(m.mean()) - p) / np.sqrt(p * (1 - p) / (B * d))
        zr = float(np.abs(m.mean(axis=1) - p).max() / np.sqrt(p * (1 - p) / d))
        zc = float(np.abs(m.mean(axis=0) - p).max() / np.sqrt(p * (1 - p) / B))
        print("[dropout] keep %.1f layer %d: overall %.2f sigma, worst row %.2f, worst column %.2f" % (kp, t, z, zr, zc))
        assert set(np.unique(m).tolist()) <= {0, 1}
        assert z <= 4.0 and zr <= 5.0 and zc <= 5.0


def test_keep_prob_one_keeps_everything():
    for m in dropout.drawn_masks(99, 5, 33, (7, 64), 1.0):
        assert m.dtype == np.uint8 and np.all(m == 1)


def test_drawn_is_a_checked_value():
    d = Drawn(99, 5)
    assert (d.seed, d.step) == (99, 5) and d == Drawn(99, 5) and d != Drawn(99, 6) and hash(d) == hash(Drawn(99, 5))
    assert Drawn(np.int64(3), np.uint64((1 << 64) - 1)).step == (1 << 64) - 1
    assert Drawn(0, 0).seed == 0
    with pytest.raises(AttributeError):
        d.step = 6
    for bad in ((1.0, 2), (1, 2.5), ('1', 2), (None, 0), (True, 0)):
        with pytest.raises(TypeError):
            Drawn(*bad)
    for bad in ((-1, 0), (0, -1), (1 << 64, 0), (0, 1 << 64)):
        with pytest.raises(ValueError):
            Drawn(*bad)
    with pytest.raises(ValueError):
        dropout.drawn_masks(-1, 0, 4, (3,), 0.5)


def test_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ipnn_hip.h")).read()
    assert re.search(r"\bint ipnn_train_step_drawn\(ipnn_handle\* h, const int32_t\* ids, const float\* wts, const float\* y, int B,\s*"
                     r"uint64_t seed, uint64_t step, float\* logits_out, float\* loss_sum_out\);", hdr)
    assert re.search(r"\bint ipnn_draw_masks\(ipnn_handle\* h, uint64_t seed, uint64_t step, int B, uint8_t\* const\* masks_out\);", hdr)
    res, args = _capi.IPNN_SIGNATURES["ipnn_train_step_drawn"]
    base = _capi.IPNN_SIGNATURES["ipnn_train_step_w"][1]
    # ipnn_train_step_w with (seed, step) where the mask array was
    assert res is C.c_int and args == base[:5] + [C.c_uint64, C.c_uint64] + base[6:]
    res, args = _capi.IPNN_SIGNATURES["ipnn_draw_masks"]
    assert res is C.c_int and args[1:3] == [C.c_uint64, C.c_uint64] and len(args) == 5


def test_library_exports_them_and_cfg_stays_96_bytes(built):
    lib = _capi.load()
    for name in NEW:
        assert getattr(lib, name).argtypes == _capi.IPNN_SIGNATURES[name][1], name
    assert lib.ipnn_cfg_size() == 96 == C.sizeof(_capi.ipnn_cfg)
