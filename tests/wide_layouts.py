"""Hand-built id layouts for the sparse-row update of WIDE rows (scatw1_form / scatw2_form of csrc/sparse_rows.hip.h): chunks of
WCH = 32 sorted entries, four sub-batches of 8 per chunk; an owner is a segment (one row's run of sorted entries) that lies in
more than one chunk -- what level 1 registers for level 2.  In the style of tests/test_gpu_scat2_forms.py (chunks of 16 there).

A field's ids are given as run lengths in SORTED position (row off + i taken lens[i] times, rows ascending), then scattered over
the examples by a seeded permutation.  One layout code per field:

  one      one row in every entry: n / 32 chunks, one owner.
  long     a run of 1040 from position 8 (33 chunks) and a run of 250 from position 10 of a later chunk (9 chunks).
  huge     a run of 6600 from position 5: 207 chunks -- at rw = 20 level 2 holds 4 * 51 = 204 chunks per trip of its stride loop.
  aligned  first half: runs of 32 on the chunk borders (no owner); second half: runs of 32 from position 16 (every run an owner
           of two chunks).
  both     a run of 70 from position 30 (two entries, two whole chunks, four entries), then runs of 24 from position 20: most
           chunks take the end of a run that entered from the left AND the opening of a run that leaves to the right, so they
           write both of their partial slots.
  sub8     runs of 8 on the sub-batch borders, then runs of 8 from position 4 (crossing 7 | 8, 15 | 16, 23 | 24 and, as an
           owner of two chunks, 31 | 32), then a pair at 31 | 32 among distinct rows.  Below 256 entries: the runs from
           position 4 alone.
  pair     distinct rows but for a pair at 31 | 32.
  deadN    N distinct live rows, ids of -1 behind them (N = 0: no live key at all; N = 1, 8, 32, 33, 40: the early exit of
           level 1 at each sub-batch and chunk border).  dead=False: further distinct rows in place of the -1.
  many     a run of 3 across every chunk border: n / 32 - 1 owners of two chunks, the most a field can register.
  zipf     Zipf(1.1) on a table of 40 rows, as a control.
"""
import numpy as np

from deep_ctr_amd import synth

WCH = 32
SPARE = 3                      # rows at the end of every field that no layout uses: they must come back bit-equal
ZIPF_ROWS = 40


def column(off, lens, n, dead):
    """A field's n entries in sorted order: row off + i taken lens[i] times, then ids of -1 -- or, dead=False, further distinct
    rows behind the live ones."""
    live = np.repeat(off + np.arange(len(lens)), lens)
    rest = np.full(n - len(live), -1) if dead else off + len(lens) + np.arange(n - len(live))
    return np.r_[live, rest].astype(np.int32)


def runs(n, length, lead):
    """Run lengths that fill n sorted positions: `lead` single entries, runs of `length`, single entries to the end."""
    k = (n - lead) // length
    return [1] * lead + [length] * k + [1] * (n - lead - k * length)


def lens_of(code, n):
    """Run lengths of layout `code` over n sorted positions; their sum is the number of live entries."""
    if code == 'one':
        return [n]
    if code == 'long':
        assert n >= 1316
        return [1] * 8 + [1040] + [1] * 18 + [250] + [1] * (n - 1316)       # 1048 + 18 = 1066 = 33 * 32 + 10
    if code == 'huge':
        assert n >= 8193
        return [1] * 5 + [6600] + [1] * (n - 6605)
    if code == 'aligned':
        assert n >= 128
        h = n // 2 // WCH * WCH
        return [WCH] * (h // WCH) + runs(n - h, WCH, 16)
    if code == 'both':
        assert n >= 256
        return [1] * 30 + [70] + [1] * 16 + runs(n - 116, 24, 0)            # 116 = 3 * 32 + 20
    if code == 'sub8':
        if n < 256:
            return runs(n, 8, 4)
        m = (n - 128) // 2 // WCH * WCH                                     # entries in runs from position 4, whole chunks
        tail = n - 64 - m
        return [8] * 8 + runs(m, 8, 4) + [1] * 31 + [2] + [1] * (tail - 33)
    if code == 'pair':
        return [1] * 31 + [2] + [1] * (n - 33)
    if code.startswith('dead'):
        live = int(code[4:])
        assert live <= n
        return [1] * live
    if code == 'many':
        q = n // WCH
        return [1] * 30 + ([3] + [1] * 29) * (q - 1) + [1] * (n - 30 - WCH * (q - 1))
    raise ValueError(code)


def field_rows(code, n, dead=True):
    """Rows a field of layout `code` needs, the SPARE untouched ones included."""
    if code == 'zipf':
        return ZIPF_ROWS + SPARE
    lens = lens_of(code, n)
    return len(lens) + (0 if dead else n - sum(lens)) + SPARE


def build(codes, n, seed, dead=True):
    """(ids int32 [n, F], sizes): field f in layout codes[f] on its own row range, which example holds which sorted entry drawn
    from `seed` (another seed: the same runs on other examples)."""
    rng = np.random.RandomState(seed)
    sizes = [field_rows(c, n, dead) for c in codes]
    off = np.r_[0, np.cumsum(sizes)]
    ids = np.empty((n, len(codes)), dtype=np.int32)
    for f, c in enumerate(codes):
        if c == 'zipf':
            ids[:, f] = off[f] + synth.zipf_ids(n, [ZIPF_ROWS], 1.1, seed + 100 + f)[:, 0]
        else:
            ids[:, f] = column(off[f], lens_of(c, n), n, dead)[rng.permutation(n)]
    return ids, sizes


def segments(col):
    """[s, e) of every row's run in the field's sorted order (ids of -1 sort to the end and are dropped)."""
    v = np.sort(col[col >= 0])
    if len(v) == 0:
        return []
    cut = np.flatnonzero(np.diff(v)) + 1
    return [(int(s), int(e)) for s, e in zip(np.r_[0, cut], np.r_[cut, len(v)])]


def owners(col):
    """(s, e, chunks) of every segment that lies in more than one chunk of 32 sorted entries: what level 1 registers."""
    return [(s, e, (e - 1) // WCH - s // WCH + 1) for s, e in segments(col) if (e - 1) // WCH > s // WCH]


def both_slots(col):
    """Chunks that write BOTH partial slots: an owner that entered from the left ends inside the chunk (slot 0) and another
    owner opens in it and runs past its end (slot 1)."""
    ow = owners(col)
    ends = set((e - 1) // WCH for s, e, c in ow if e % WCH != 0)            # e on the border: slot 0 of a full chunk, no room to open
    opens = set(s // WCH for s, e, c in ow)
    return sorted(ends & opens)


def whole_chunks(col):
    """Chunks that a segment covers without starting or ending in them."""
    return sorted(q for s, e, c in owners(col) for q in range(s // WCH + 1, (e - 1) // WCH))


def live_count(col):
    return int((col >= 0).sum())


# The cases of tests/test_gpu_wide_rows_exact.py: (k, B, max_batch, one layout code per field, precision, steps).  N2 = 256 at
# B = 40; 4096 without a padding key; 4097 the smallest batch on N2 = 8192; 8193 the smallest on 16384; 16384 without a padding
# key (512 chunks per field).  k = 17..20: rw = 20 with pads 3, 2, 1, 0 (nq = 5, ngrp = 51, one idle thread in level 2);
# k = 128: nq = 32, ngrp = 8 (`one` at 16384: 16 trips of level 2); k = 101 on 39 fields: F * rw = 4056, the largest.
CYCLE39 = ['one', 'long', 'both', 'sub8', 'dead33', 'many', 'aligned', 'zipf', 'dead0', 'pair', 'dead8', 'many', 'dead32']
EXACT = [
    (17, 40, 256, ['one', 'sub8', 'dead33', 'pair'], 'f32', 2),
    (18, 40, 256, ['dead0', 'dead1', 'dead8', 'dead40'], 'f32', 1),
    (19, 40, 256, ['dead32', 'one', 'sub8', 'dead0'], 'f32', 1),
    (18, 4096, 4096, ['one', 'long', 'both', 'many'], 'f32', 2),
    (20, 4096, 4096, ['many', 'many', 'many', 'aligned'], 'f32', 1),
    (19, 4097, 8192, ['one', 'sub8', 'many', 'zipf'], 'f32', 1),
    (17, 8192, 8192, ['many', 'many', 'many', 'long'], 'bf16', 1),
    (20, 8193, 16384, ['huge', 'one', 'both'], 'f32', 1),
    (20, 16384, 16384, ['huge', 'one', 'aligned', 'many'], 'f32', 1),
    (18, 16384, 16384, ['one', 'huge', 'both', 'dead8'], 'f32', 1),
    (128, 16384, 16384, ['one', 'long', 'dead40'], 'f32', 1),
    (128, 4096, 4096, ['one', 'both', 'sub8', 'long'], 'bf16x3', 1),
    (101, 4096, 4096, [CYCLE39[f % len(CYCLE39)] for f in range(39)], 'f32', 1),
]
# The layouts of tests/test_gpu_wide_rows_plain.py (the plain form at its consumers): B = 4096 on N2 = 4096, and B = 40.
PLAIN_BIG = ['one', 'long', 'both', 'sub8', 'dead33', 'many', 'many', 'many']
PLAIN_SMALL = ['one', 'sub8', 'dead33', 'pair', 'dead0', 'dead8']


def exact_id(case):
    K, B, mb, codes, prec, steps = case
    return 'K%d-B%d-of-%d-%s-%s-%dstep' % (K, B, mb, '+'.join(codes) if len(codes) <= 4 else '%dfields' % len(codes), prec, steps)
