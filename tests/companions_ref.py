"""numpy restatement of the companion-utterance contract (include/fakebob_hip.h: fb_set_companions -- "Composition", "Row
order", "Averaging"), written from the header and from nothing else.  It puts the composition and the row order on top of
tests/input_transform_ref.py / tests/input_transform_noise_ref.py (the chain) and the averaging on top of eot_mean.

    w[b][0]   = q_b                                           the NES row itself
    w[b][u]   = clip(a_u + q_b - a_0, -32768, 32767)          int32 arithmetic, u = 1 .. K1
    replica rho = u * r + j of row b  ->  row b * K * r + rho;  rho is the noise contract's `replica`
    an SNR stage's E is the power of the composed row (b, u)
    loss[b]   = (l[b][0] + ... + l[b][K r - 1]) / (K r)       float64, rho ascending: eot_mean over the replicas

The normals are an ARGUMENT, as in input_transform_noise_ref.py: normals(b, rho, s) -> the float32 normals stage s adds to
NES row b's replica rho (the generator has its own contract and tests)."""
import numpy as np

from tests.input_transform_noise_ref import NOISE, eot_mean, ref_noisy


def compose_row(q, a0, companions):
    """The K composed utterances of one NES row: q (N,) int16, a0 (N,) int16, companions (K1, N) int16 -> (K, N) int16"""
    q, a0 = np.asarray(q), np.asarray(a0)
    assert q.dtype == np.int16 and a0.dtype == np.int16 and q.shape == a0.shape and q.ndim == 1
    rows = [q.copy()]                                   # utterance 0: q itself
    for a in np.asarray(companions).reshape(-1, q.size):
        assert a.dtype == np.int16
        v = a.astype(np.int32) + q.astype(np.int32) - a0.astype(np.int32)
        rows.append(np.clip(v, -32768, 32767).astype(np.int16))
    return np.stack(rows)


def compose(q, a0, companions, chain, r, normals=None):
    """What the composing launch writes: q (B, N) -> (B, K, r, N); row b * K * r + u * r + j of the flat batch is [b][u][j].
    chain: (kind, k, taps) stages; normals(b, rho, s) as above (needed for noise stages only)."""
    q = np.asarray(q)
    out = []
    for b in range(q.shape[0]):
        w = compose_row(q[b], a0, companions)
        rows = []
        for u in range(w.shape[0]):
            reps = []
            for j in range(r):
                rho = u * r + j
                z = {s: normals(b, rho, s) for s, st in enumerate(chain) if st[0] == NOISE}
                reps.append(ref_noisy(w[u], chain, z))      # (E: the power of w[u], the chain's input)
            rows.append(np.stack(reps))
        out.append(np.stack(rows))
    return np.stack(out)


def mean_over_replicas(v):
    """The contract's averaging over the LAST axis (the K * r replicas of a row, rho ascending): eot_mean's rule"""
    return eot_mean(v)
