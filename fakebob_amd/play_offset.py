"""Play offset: the perturbation plays on a loop and the victim speaks whenever they speak (fb_set_play_offset; the "Play
offset" section of include/fakebob_hip.h).  The host side of the contract: the draw of an offset, the composition of a
rotated perturbation onto a recording, the grid of offsets an attack's result is re-scored on, and the argument handling of
FakeBob(play_offset=...) / attack_main --play-offset.  Nothing here runs on the hot path: the offsets inside an attack are
drawn and applied by the library (k_play_compose)."""
import numpy as np

from .companions import cast_i16

MAX_OFFSET = 2 ** 31 - 2      # fb_set_play_offset: 0 <= S <= 2^31 - 2
PLAY = 0x504C4159             # "PLAY": the key of the offsets' Philox stream is (seed_lo ^ PLAY, seed_hi ^ stream)
GRID = 16                     # offsets an attack's result is re-scored on (AttackResult.per_offset)
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3"): four counter words, two key words ->
    four output words."""
    c0, c1, c2, c3 = (int(c) & _M32 for c in counter)
    k0, k1 = (int(k) & _M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> 32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return [c0, c1, c2, c3]


def check_offset(S):
    """S as fb_set_play_offset takes it: None -> 0; ValueError outside 0 .. 2^31 - 2."""
    S = 0 if S is None else int(S)
    if not 0 <= S <= MAX_OFFSET:
        raise ValueError("play offset %d outside 0 .. 2^31 - 2" % S)
    return S


def draw(seed, stream, epoch, b, rho, S):
    """The offset of replica rho of utterance row b at (seed, stream, epoch): word 0 of Philox on the "PLAY" key at counter
    (0, rho, b, epoch), scaled to 0 .. S."""
    S = check_offset(S)
    seed = int(seed)
    key = [(seed & _M32) ^ PLAY, ((seed >> 32) & _M32) ^ (int(stream) & _M32)]
    w = philox4x32_10([0, int(rho), int(b), int(epoch)], key)[0]
    return (w * (S + 1)) >> 32


def compose(host_i16, delta_i16, tau):
    """The contract's composition on the host: out[i] = clip(host[i] + delta[(i - tau) mod N], -32768, 32767), int32
    arithmetic -> int16.  delta: the perturbation adv_i16 - a_0 (any integer dtype; a difference of two int16)."""
    a = np.asarray(host_i16)
    if a.dtype != np.int16:
        raise ValueError("the host recording must be int16 (fakebob_amd.companions.cast_i16)")
    a = a.reshape(-1)
    d = np.asarray(delta_i16).reshape(-1).astype(np.int32)
    if d.size != a.size:
        raise ValueError("utterance of %d samples, perturbation of %d" % (a.size, d.size))
    tau = int(tau)
    if not 0 <= tau < a.size:
        raise ValueError("offset %d outside the loop of %d samples" % (tau, a.size))
    return np.clip(a.astype(np.int32) + np.roll(d, tau), -32768, 32767).astype(np.int16)


def apply_perturbation(perturbation, wavs, offset=0, bits_per_sample=16):
    """companions.apply_perturbation with the perturbation rotated by `offset`: a list of int16 arrays."""
    if isinstance(wavs, np.ndarray) and wavs.ndim == 1:
        wavs = [wavs]
    return [compose(cast_i16(w, bits_per_sample), perturbation, offset) for w in wavs]


def offset_grid(S, n=GRID):
    """n evenly spaced offsets over 0 .. S, both ends included (fewer when S + 1 < n: every offset once), ascending ints."""
    S = check_offset(S)
    n = int(n)
    if n < 2:
        raise ValueError("a grid needs both ends: n >= 2")
    if S + 1 <= n:
        return list(range(S + 1))
    return [(k * S) // (n - 1) for k in range(n)]


def per_offset(model, task, attack_type, hosts, delta, S, target=None, true=None, **score_kw):
    """AttackResult.per_offset: for each int16 recording of `hosts` (utterance 0 first) the perturbation `delta` rotated by each
    offset of offset_grid(S), composed onto it and decided by the system's ordinary model.make_decisions -> one dict per
    utterance: utterance, offsets, decisions, successes (booleans), n_success."""
    from .companions import succeeded
    grid = offset_grid(S)
    out = []
    for u, host in enumerate(hosts):
        decs = [model.make_decisions(compose(host, delta, t), **score_kw)[0] for t in grid]
        ok = [bool(succeeded(task, attack_type, d, target=target, true=true)) for d in decs]
        out.append(dict(utterance=u, offsets=list(grid), decisions=decs, successes=ok, n_success=int(sum(ok))))
    return out


def parse_option(text, n_samples):
    """attack_main's --play-offset: "max" -> n_samples - 1 (the whole loop), else an integer 0 .. n_samples - 1."""
    if text is None:
        return 0
    t = str(text).strip().lower()
    S = int(n_samples) - 1 if t == "max" else check_offset(int(t))
    if S >= int(n_samples):
        raise ValueError("--play-offset %d: the utterance has %d samples, the offset must stay below that" % (S, n_samples))
    return S
