"""The dropout keep-masks the inner-product family draws on the device (ipnn_train_step_drawn / ipnn_draw_masks,
include/ipnn_hip.h), restated in NumPy: the same bits, for replaying a step in the oracle.  NumPy only.

The draw is a pure function of (seed, step, layer, example, column): Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel
random numbers: as easy as 1, 2, 3", SC'11) under

    key     = (lo32(seed), hi32(seed))
    counter = (c, (t << 16) | (ex >> 2), lo32(step), hi32(step))
    word j (0..3) of the output belongs to example 4 * (ex >> 2) + j
    keep    = word < min(2^32 - 1, floor((double)(float)keep_prob * 2^32));   keep_prob >= 1 keeps every element

for layer t = 0..n_hidden, example ex and column c in the reference's column order (layer 0: [e | pairs | b]).  seed and step
are uint64, any value.  The mask of an element depends on neither the batch size nor the layer's width."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # the key bumps (golden ratio, sqrt(3) - 1)
_U64 = (1 << 64) - 1
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: 4 values, key: 2 values (ints or integer arrays that broadcast against each other, each below 2^32).
    Returns uint32 [..., 4]: the four output words of ten rounds."""
    c = [np.asarray(x).astype(np.uint64) for x in counter]
    k = [np.asarray(x).astype(np.uint64) for x in key]
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(c + k))
    m0, m1, w0, w1 = np.uint64(M0), np.uint64(M1), np.uint64(W0), np.uint64(W1)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                       # 32 x 32 -> 64 bits: never wraps in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0, k1 = (k0 + w0) & _LO, (k1 + w1) & _LO
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _u64(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError("%s must be an integer, not %r" % (name, type(v).__name__))
    v = int(v)
    if not 0 <= v <= _U64:
        raise ValueError("%s = %d is outside uint64" % (name, v))
    return v


def threshold(keep_prob):
    """The 32-bit threshold of a keep probability (the float32 the C ABI carries), or None: keep everything."""
    kp = float(np.float32(keep_prob))
    if kp >= 1.0:
        return None
    return min((1 << 32) - 1, int(np.floor(kp * 4294967296.0)))


def drawn_masks(seed, step, B, d, keep_prob):
    """The keep-masks of step `step` under `seed`: a list of uint8 [B, d[t]], t = 0..len(d)-1 -- what ipnn_draw_masks writes
    for a handle whose layers have d[t] columns (IPNNEngine.d[:-1])."""
    seed, step = _u64('seed', seed), _u64('step', step)
    thr = threshold(keep_prob)
    out = []
    g = np.arange((B + 3) // 4, dtype=np.uint64)[:, None]
    for t, dt in enumerate(d):
        if thr is None:
            out.append(np.ones((B, dt), np.uint8))
            continue
        col = np.arange(dt, dtype=np.uint64)[None, :]
        w = philox4x32_10((col, np.uint64(t << 16) | g, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        # w [groups, dt, 4]: word j of group g is example 4 g + j
        m = (w < np.uint32(thr)).astype(np.uint8).transpose(0, 2, 1).reshape(-1, dt)
        out.append(np.ascontiguousarray(m[:B]))
    return out
