"""The layouts of tests/wide_layouts.py have the properties the GPU cases name (tests/test_gpu_wide_rows_exact.py,
tests/test_gpu_wide_rows_plain.py): owner counts, chunks per owner, the chunks that write both partial slots, live counts, ids
inside their field's row range.  No GPU: if a layout drifts, this fails here and the GPU cases cannot silently stop hitting the
chunk borders, trip counts and owner counts they are there for."""
import numpy as np
import pytest

from deep_ctr_amd import synth

import wide_layouts as wl
from wide_layouts import WCH, both_slots, live_count, owners, segments, whole_chunks

SIZES = (40, 4096, 4097, 8192, 8193, 16384)


def col(code, n, seed=1, dead=True):
    ids, sizes = wl.build([code], n, seed, dead)
    return ids[:, 0]


def trips(chunks, rw):
    """Trips of level 2's stride loop for an owner of `chunks` chunks: 4 * ngrp chunks per trip, ngrp = 256 / (rw / 4)."""
    per = 4 * (256 // (rw // 4))
    return (chunks + per - 1) // per


@pytest.mark.parametrize("n", SIZES)
def test_one(n):
    c = col('one', n)
    assert live_count(c) == n and len(segments(c)) == 1
    assert owners(c) == [(0, n, (n + WCH - 1) // WCH)]
    assert len(whole_chunks(c)) == (n + WCH - 1) // WCH - 2
    if n == 16384:
        assert owners(c)[0][2] == 512 and trips(512, 128) == 16 and trips(512, 20) == 3


@pytest.mark.parametrize("n", SIZES[1:])
def test_long(n):
    c = col('long', n)
    assert live_count(c) == n
    assert owners(c) == [(8, 1048, 33), (1066, 1316, 9)] and 1066 % WCH == 10
    assert trips(33, 20) == 1 and trips(33, 104) == 1 and trips(33, 128) == 2 and trips(33, 316) == 3    # ngrp = 3: 12 chunks a trip
    assert trips(33, 192) == 2                                                                      # the bag table at h0 = 192: ngrp = 5


@pytest.mark.parametrize("n", (8193, 16384))
def test_huge_takes_the_second_trip_of_level_2_at_rw_20(n):
    c = col('huge', n)
    assert live_count(c) == n
    assert owners(c) == [(5, 6605, 207)]
    assert 207 > 4 * (256 // 5) and trips(207, 20) == 2
    with pytest.raises(AssertionError):
        wl.lens_of('huge', 8192)


@pytest.mark.parametrize("n", SIZES[1:])
def test_aligned(n):
    c = col('aligned', n)
    h = n // 2 // WCH * WCH
    seg = segments(c)
    assert live_count(c) == n
    first = [(s, e) for s, e in seg if e <= h]
    assert first == [(q * WCH, (q + 1) * WCH) for q in range(h // WCH)]            # whole chunks: no owner, no partial slot
    ow = owners(c)
    assert len(ow) == (n - h - 16) // WCH and len(ow) >= 63
    assert all(cc == 2 and e - s == WCH and s % WCH == 16 and s >= h for s, e, cc in ow)
    assert both_slots(c) == sorted(s // WCH + 1 for s, e, cc in ow[:-1])         # a run ends at 16, the next opens at 16


@pytest.mark.parametrize("n", SIZES[1:])
def test_both(n):
    c = col('both', n)
    assert live_count(c) == n
    ow = owners(c)
    assert ow[0] == (30, 100, 4) and whole_chunks(c) == [1, 2]                    # two whole middle chunks
    assert all(e - s == 24 and s % 24 == 116 % 24 and cc == 2 for s, e, cc in ow[1:])
    bs = both_slots(c)
    assert len(bs) >= 1 and 3 in bs and 4 in bs          # chunk 3: the run of 70 ends at 100, 116..140 opens; chunk 4: 116..140 ends, 140..164 opens
    assert len(bs) > n // WCH // 2
    inside = [(s, e) for s, e in segments(c) if e - s == 24 and s // WCH == (e - 1) // WCH]
    assert len(inside) > 0                                # and runs of 24 that stay inside one chunk (32 - 24 = 8: positions 0..8)


@pytest.mark.parametrize("n", SIZES)
def test_sub8(n):
    c = col('sub8', n)
    assert live_count(c) == n
    seg = segments(c)
    ow = owners(c)
    if n < 256:
        assert seg[:4] == [(0, 1), (1, 2), (2, 3), (3, 4)] and seg[4:8] == [(4, 12), (12, 20), (20, 28), (28, 36)]
        assert ow == [(28, 36, 2)]
        return
    assert seg[:8] == [(8 * i, 8 * i + 8) for i in range(8)]                      # on the sub-batch borders
    m = (n - 128) // 2 // WCH * WCH
    shifted = [(s, e) for s, e in seg if e - s == 8 and s >= 64]
    assert len(shifted) == (m - 4) // 8 and all(s % 8 == 4 and 64 <= s and e <= 64 + m for s, e in shifted)
    assert set(s % WCH for s, e in shifted) == {4, 12, 20, 28}                   # across 7 | 8, 15 | 16, 23 | 24 and 31 | 32
    cross = [(s, e, cc) for s, e, cc in ow if e - s == 8]
    assert len(cross) == m // WCH - 1 and all(s % WCH == 28 and cc == 2 for s, e, cc in cross)
    pair = [(s, e, cc) for s, e, cc in ow if e - s == 2]
    assert pair == [(64 + m + 31, 64 + m + 33, 2)] and (64 + m) % WCH == 0       # the pair at 31 | 32
    assert len(ow) == len(cross) + 1
    assert seg[-1] == (n - 1, n)                                                  # distinct rows behind the pair


@pytest.mark.parametrize("n", SIZES)
def test_pair(n):
    c = col('pair', n)
    assert live_count(c) == n and owners(c) == [(31, 33, 2)] and len(segments(c)) == n - 1


@pytest.mark.parametrize("live", (0, 1, 8, 32, 33, 40))
@pytest.mark.parametrize("n", (40, 4096))
def test_dead(n, live):
    c = col('dead%d' % live, n)
    assert live_count(c) == live and int((c == -1).sum()) == n - live
    assert owners(c) == [] and len(segments(c)) == live                           # distinct rows
    full = col('dead%d' % live, n, dead=False)                                    # the inner-product step refuses ids of -1
    assert full.min() >= 0 and len(segments(full)) == n and owners(full) == []
    # where level 1 leaves: live = 0: at once, in every chunk; 1: inside the first sub-batch; 8, 32: on a sub-batch / chunk
    # border; 33, 40: the second chunk, inside / on the border of its first sub-batch
    first_dead = (live // WCH, live % WCH // 8, live % 8)                         # (chunk, sub-batch of 8, entry) of the first id of -1
    assert first_dead == {0: (0, 0, 0), 1: (0, 0, 1), 8: (0, 1, 0), 32: (1, 0, 0), 33: (1, 0, 1), 40: (1, 1, 0)}[live]


@pytest.mark.parametrize("n", SIZES[1:])
def test_many(n):
    c = col('many', n)
    assert live_count(c) == n
    ow = owners(c)
    assert len(ow) == n // WCH - 1                                                # one owner per chunk border
    assert all(e - s == 3 and s % WCH == 30 and cc == 2 for s, e, cc in ow)
    assert both_slots(c) == list(range(1, n // WCH - 1))                          # the end of one run of 3, the opening of the next


def test_zipf():
    for n in (4097, 4096):
        c = col('zipf', n)
        assert live_count(c) == n and len(segments(c)) <= wl.ZIPF_ROWS
        assert max(e - s for s, e in segments(c)) > 5 * WCH                       # runs over several chunks, of every length


def check_case(codes, n, seed, dead=True):
    """Every id in its field's row range, the SPARE rows of every field untouched; -> owners per field."""
    ids, sizes = wl.build(codes, n, seed, dead)
    fo = synth.field_of_row(sizes)
    off = np.r_[0, np.cumsum(sizes)]
    assert ids.shape == (n, len(codes)) and ids.dtype == np.int32
    for f, code in enumerate(codes):
        live = ids[:, f][ids[:, f] >= 0]
        assert np.all(fo[live] == f), (code, f)
        assert live.size == 0 or live.max() < off[f + 1] - wl.SPARE, (code, f)
        if dead is False:
            assert live.size == n
    other, _ = wl.build(codes, n, seed + 1, dead)
    assert not np.array_equal(ids, other)                                         # another seed: other examples ...
    assert all(np.array_equal(np.sort(ids[:, f]), np.sort(other[:, f])) for f in range(len(codes)) if codes[f] != 'zipf')   # ... the same runs
    return [len(owners(ids[:, f])) for f in range(len(codes))]


def test_exact_cases_reach_what_they_name():
    seen_k, seen_b, over256, over512 = set(), set(), 0, 0
    for case in wl.EXACT:
        K, B, mb, codes, prec, steps = case
        n_own = check_case(codes, B, 11)
        N2 = 256
        while N2 < B:
            N2 *= 2
        assert B <= mb and N2 == max(256, mb), case                               # the handle's own slot, at its full N2
        seen_k.add(K); seen_b.add((B, mb))
        many = [n for n, c in zip(n_own, codes) if c == 'many']
        if len(many) >= 3:
            over256 += sum(many[:3]) > 256
            over512 += sum(many[:3]) > 512
        if 'huge' in codes:
            assert B >= 8193 and (K + 3) // 4 * 4 == 20                           # the second trip at rw = 20
        if len(codes) == 39:
            assert K == 101 and 39 * 104 == 4056 and set(codes) == set(wl.CYCLE39)
            assert sum(n_own) > 256
    assert seen_k == {17, 18, 19, 20, 101, 128}                                    # pads 3, 2, 1, 0 at rw = 20; 3; 0
    assert seen_b == {(40, 256), (4096, 4096), (4097, 8192), (8192, 8192), (8193, 16384), (16384, 16384)}
    assert over256 >= 2 and over512 >= 1                                          # level 2's `o += nblk` at 256 workgroups: two and three rounds
    assert sorted(set(c[4] for c in wl.EXACT)) == ['bf16', 'bf16x3', 'f32']
    assert sum(c[5] == 2 for c in wl.EXACT) == 2
    one20 = [c for c in wl.EXACT if c[1] == 16384 and c[0] <= 20 and 'one' in c[3] and 'huge' in c[3]]
    one128 = [c for c in wl.EXACT if c[1] == 16384 and c[0] == 128 and 'one' in c[3]]
    assert one20 and one128


def test_plain_cases_reach_what_they_name():
    for dead in (True, False):
        n_own = check_case(wl.PLAIN_BIG, 4096, 21, dead)
        assert sum(n for n, c in zip(n_own, wl.PLAIN_BIG) if c == 'many') == 3 * 127 > 256
        check_case(wl.PLAIN_SMALL, 40, 22, dead)
    ids, _ = wl.build(wl.PLAIN_BIG, 4096, 21)
    assert len(both_slots(ids[:, wl.PLAIN_BIG.index('both')])) > 0
    assert live_count(ids[:, wl.PLAIN_BIG.index('dead33')]) == 33
    small, _ = wl.build(wl.PLAIN_SMALL, 40, 22)
    assert live_count(small[:, wl.PLAIN_SMALL.index('dead0')]) == 0
    assert owners(small[:, 0]) == [(0, 40, 2)]
