"""numpy restatement of the feature-compression stage (fb_set_feature_compression), written from the stage contract in
include/fakebob_hip.h and nothing else: keys -> selection -> Lloyd iterations, the distance accumulated dimension by
dimension in float32, the update a float64 loop over the frames in ascending order.  `philox(counter[4], key[2]) -> 4 words`
is handed in (oracle.philox), so this module needs no library."""
import numpy as np

FECO = 0x4645434F
M32 = 0xFFFFFFFF


def feco_k(T, ratio):
    """k = max(1, (int)floor((double)T * ratio)); T = 0 gives 0"""
    if T <= 0:
        return 0
    return max(1, int(np.floor(np.float64(T) * np.float64(ratio))))


def feco_keys(philox, seed, stream, epoch, utt, replica, T):
    """key of frame t = word t & 3 of Philox4x32-10, key (seed_lo ^ "FECO", seed_hi ^ stream), counter (t >> 2, 0x100 +
    replica, utterance row, epoch)"""
    key = [(seed & M32) ^ FECO, ((seed >> 32) & M32) ^ (stream & M32)]
    out = np.empty(T, np.uint32)
    for q in range((T + 3) // 4):
        w = philox([q, 0x100 + replica, utt & M32, epoch & M32], key)
        for i in range(4):
            if 4 * q + i < T:
                out[4 * q + i] = w[i]
    return out


def feco_init(keys, k):
    """the k frames of smallest (key, t), in ascending t"""
    order = sorted(range(len(keys)), key=lambda t: (int(keys[t]), t))
    return sorted(order[:k])


def feco_assign(X, C):
    """labels[t] = the centre of smallest d(t, j), the lowest j on a tie; d accumulated in float32 from 0 over the dimensions in
    ascending order: diff = x - c, sq = diff * diff, acc = acc + sq, each one float32 operation"""
    T, D = X.shape
    acc = np.zeros((T, C.shape[0]), np.float32)
    for d in range(D):
        diff = X[:, d, None] - C[None, :, d]
        assert diff.dtype == np.float32
        sq = diff * diff
        acc = acc + sq
    assert acc.dtype == np.float32
    return np.argmin(acc, axis=1)            # (the first smallest; the tests feed no NaN)


def feco_update(X, C, labels):
    """a centre with members = (float)(S / n), S the float64 sum of its members' rows in ascending t from 0.0; one without
    keeps its value"""
    k, D = C.shape
    S = np.zeros((k, D), np.float64)
    n = np.zeros(k, np.int64)
    for t in range(X.shape[0]):
        S[labels[t]] = S[labels[t]] + X[t].astype(np.float64)
        n[labels[t]] += 1
    out = C.copy()
    for j in range(k):
        if n[j] > 0:
            out[j] = (S[j] / np.float64(n[j])).astype(np.float32)
    return out


def feco(X, keys, ratio, iters, init=None):
    """X (T, D) float32, keys (T,) uint32 -> (centres (k, D) float32, labels of the last assignment).  init: the initial
    centres' frames instead of the keyed choice (the host tests).  Stops once an iteration changes no assignment, which the
    contract allows."""
    X = np.ascontiguousarray(X, np.float32)
    T = X.shape[0]
    k = feco_k(T, ratio)
    if k == 0:
        return X[:0].copy(), np.zeros(0, np.int64)
    idx = feco_init(keys, k) if init is None else list(init)
    assert len(idx) == k
    C = X[idx].copy()
    labels = None
    for it in range(iters):
        new = feco_assign(X, C)
        if labels is not None and np.array_equal(new, labels):
            break
        labels = new
        C = feco_update(X, C, labels)
    return C, labels


def feco_batch(philox, mats, r, seed, stream, epoch, ratio, iters, utt0=0):
    """what Engine.debug_feature_compress returns: for every matrix the centres under replicas 0 .. r - 1"""
    out = []
    for b, X in enumerate(mats):
        X = np.ascontiguousarray(X, np.float32)
        out.append([feco(X, feco_keys(philox, seed, stream, epoch, utt0 + b, j, X.shape[0]), ratio, iters)[0] for j in range(r)])
    return out
