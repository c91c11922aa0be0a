"""numpy restatement of the play-offset contract (include/fakebob_hip.h: fb_set_play_offset -- "Draw", "Composition", "Row
order", "Transposed rule"), written from the header and from nothing else.  It puts the offset on top of
tests/companions_ref.py's row order and tests/input_transform_noise_ref.py's chain.

    tau(b, rho)   = (w * (S + 1)) >> 32, w = word 0 of Philox(counter (0, rho, b, epoch), key (seed_lo ^ "PLAY", seed_hi ^ stream))
    w[b][rho][i]  = clip(a_u[i] + d_b[(i - tau) mod N], -32768, 32767), d_b = q_b - a_0, u = rho // eot, EVERY u
    grad[k]       = sum over rho ascending of m_rho[i] * cot_rho[i] at i = (k + tau_rho) mod N, float64 from +0.0

`philox(counter[4], key[2]) -> 4 words` is handed in (oracle.philox), as in tests/pso_ref.py: this module needs no library.
The normals of noise stages are an argument, as in tests/companions_ref.py."""
import numpy as np

from tests.input_transform_noise_ref import NOISE, ref_noisy

PLAY = 0x504C4159
M32 = 0xFFFFFFFF
TILE = 2048          # samples of a k_play_compose workgroup's tile (256 lanes x 8 samples; play_offset_kernels.hip)


def play_key(seed, stream):
    return [(seed & M32) ^ PLAY, ((seed >> 32) & M32) ^ (stream & M32)]


def draw(philox, seed, stream, epoch, b, rho, S):
    w = int(philox([0, rho, b, epoch & M32], play_key(seed, stream))[0])
    return (w * (S + 1)) >> 32


def offsets(philox, seed, stream, epoch, B, r, S, utt0=0):
    """tau [B][r]: replica rho of utterance row utt0 + b"""
    return np.array([[draw(philox, seed, stream, epoch, utt0 + b, rho, S) for rho in range(r)] for b in range(B)], np.int64)


def compose_one(host, q, a0, tau):
    """clip(host[i] + (q - a0)[(i - tau) mod N]) -> int16"""
    host, q, a0 = np.asarray(host), np.asarray(q), np.asarray(a0)
    assert host.dtype == np.int16 and q.dtype == np.int16 and a0.dtype == np.int16 and host.shape == q.shape == a0.shape and q.ndim == 1
    assert 0 <= tau < q.size
    d = q.astype(np.int32) - a0.astype(np.int32)
    idx = (np.arange(q.size) - int(tau)) % q.size
    return np.clip(host.astype(np.int32) + d[idx], -32768, 32767).astype(np.int16)


def hosts(a0, companions):
    """a_u, u = 0 .. K - 1: a_0 and the companions, (K, N) int16"""
    a0 = np.asarray(a0)
    comp = np.zeros((0, a0.size), np.int16) if companions is None else np.asarray(companions).reshape(-1, a0.size)
    assert comp.dtype == np.int16
    return np.concatenate([a0[None], comp])


def compose_rows(q, a0, companions, eot, tau):
    """The K * eot composed rows of ONE NES row under the offsets tau [K * eot]: (K * eot, N) int16, row rho = u * eot + j"""
    h = hosts(a0, companions)
    return np.stack([compose_one(h[rho // eot], q, a0, int(tau[rho])) for rho in range(h.shape[0] * eot)])


def compose(q, a0, companions, chain, eot, tau, normals=None):
    """What k_play_compose and the chain behind it write: q (B, N), tau (B, K * eot) -> (B, K, eot, N).  An SNR stage's E is
    the power of the composed, OFFSET row."""
    q = np.asarray(q)
    out = []
    for b in range(q.shape[0]):
        w = compose_rows(q[b], a0, companions, eot, tau[b])
        rows = []
        for rho in range(w.shape[0]):
            z = {s: normals(b, rho, s) for s, st in enumerate(chain) if st[0] == NOISE}
            rows.append(ref_noisy(w[rho], chain, z))
        out.append(np.stack(rows).reshape(-1, eot, q.shape[1]))
    return np.stack(out)


def mask(q, a0, companions, eot, tau):
    """m [K * eot][N]: 1 where a_u[i] + d[(i - tau_rho) mod N], before the clip, lies inside the int16 range"""
    h = hosts(a0, companions).astype(np.int64)
    d = np.asarray(q).astype(np.int64) - np.asarray(a0).astype(np.int64)
    n = d.size
    m = []
    for rho in range(h.shape[0] * eot):
        v = h[rho // eot] + d[(np.arange(n) - int(tau[rho])) % n]
        m.append((v >= -32768) & (v <= 32767))
    return np.stack(m)


def compose_t(cot, q, a0, companions, eot, tau):
    """The transposed rule: cot (K * eot, N) float64 -> grad (N,) float64, rho ascending from +0.0, a masked term adds +0.0"""
    cot = np.asarray(cot, np.float64)
    m = mask(q, a0, companions, eot, tau)
    n = cot.shape[1]
    acc = np.zeros(n, np.float64)
    k = np.arange(n)
    for rho in range(cot.shape[0]):
        i = (k + int(tau[rho])) % n
        acc = acc + np.where(m[rho, i], cot[rho, i], 0.0)
    return acc


def compose_linear(delta, q, a0, companions, eot, tau):
    """The derivative of the composition at q applied to an integer direction delta (N,): row rho is m_rho[i] *
    delta[(i - tau_rho) mod N] -- what the adjoint identity pairs compose_t with; exact in int64"""
    m = mask(q, a0, companions, eot, tau)
    delta = np.asarray(delta, np.int64)
    n = delta.size
    return np.stack([np.where(m[rho], delta[(np.arange(n) - int(tau[rho])) % n], 0) for rho in range(m.shape[0])])


def wraps_inside_a_tile(n, R, tau, tile=TILE):
    """whether the wrap of offset tau in row R of the flat batch -- output sample i = tau, where the rotated source jumps from
    n - 1 back to 0 -- falls strictly inside a workgroup's tile: the launch cuts the flat array [rows * n] into chunks of eight
    samples, row R's workgroups take the chunks that start in it, tile / 8 per workgroup; strictly inside = neither in the
    first nor in the last chunk of a workgroup, nor in the row's first or last chunk"""
    if not 0 < tau < n:
        return False
    per = tile // 8
    c_lo, c_hi = (R * n + 7) // 8, ((R + 1) * n + 7) // 8
    c = (R * n + tau) // 8
    if not c_lo < c < c_hi - 1:
        return False
    lane = (c - c_lo) % per
    return 0 < lane < per - 1
