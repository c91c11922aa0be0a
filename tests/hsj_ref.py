"""HopSkipJump restated in numpy: the "decision-only attack II" section of include/fakebob_hip.h, operation by operation.

Every float64 operation is one numpy ufunc call (one IEEE rounding, no fused multiply-add), in the order the contract
writes them, so the values are the device's bit for bit.  The normals are an argument: `noise(seed, t, stream, N, B)` ->
float32 (B, N), the NES generator's rows for iteration t under `seed` (the tests pass oracle.noise; the probes' key is
seed ^ KEY).  `drive` replays a whole attack from a decision log, or runs one against a victim given as a function."""
import math

import numpy as np

KEY = 0x48534A50          # "HSJP"
Q = 1 << 20
DEFAULTS = dict(grid=15, max_rounds=8, num_evals_init=32, num_evals_max=256, max_queries=0, sigma_min=2.0 ** -15,
                probe_scale=0.05)


def cast_i16(x, bits=16):
    """the engine's int16 cast: trunc(x * 2^(bits - 1)), the low 16 bits"""
    v = np.trunc(np.asarray(x, np.float64) * float(2 ** (bits - 1))).astype(np.int64)
    return (v & 0xFFFF).astype(np.uint16).view(np.int16)


def clip1(s):
    return np.minimum(np.maximum(s, -1.0), 1.0)


def ssq_parts(v):
    """the chunk sums P_c of ssq(v)"""
    v = np.asarray(v, np.float64).reshape(-1)
    chunks = max(-(-v.size // 1024), 1)
    p = np.zeros(chunks * 1024, np.float64)
    p[:v.size] = v
    p = p.reshape(chunks, 256, 4)
    sq = p * p
    s = ((sq[:, :, 0] + sq[:, :, 1]) + sq[:, :, 2]) + sq[:, :, 3]
    stride = 128
    while stride >= 1:
        s[:, :stride] = s[:, :stride] + s[:, stride:2 * stride]
        stride //= 2
    return s[:, 0].copy()


def ssq(v):
    acc = 0.0
    for pc in ssq_parts(v):
        acc = acc + float(pc)
    return acc


def line(a, y, q):
    """a + (q 2^-20) (y - a): the difference, the exact scale, the product, the sum"""
    a, y = np.asarray(a, np.float64), np.asarray(y, np.float64)
    sc = np.float64(int(q)) * np.float64(2.0 ** -20)
    return a + sc * (y - a)


def num_evals(params, t):
    return min(params["num_evals_max"], math.isqrt(params["num_evals_init"] ** 2 * t))


def sigma_of(params, dist, n):
    return max(params["sigma_min"], (params["probe_scale"] * dist) / math.sqrt(float(n)))


def probes(x, sigma, z, bits=16):
    """rows (B, N) int16: the cast of clip(x + sigma z_j, -1, 1); z float32 (B, N)"""
    x = np.asarray(x, np.float64)
    return cast_i16(clip1(x[None, :] + np.float64(sigma) * np.asarray(z, np.float32).astype(np.float64)), bits)


def weights(flags):
    """the integer weights of the adversarial flags of an iteration's probes -> (w int32 (B,), n+)"""
    phi = np.where(np.asarray(flags, bool), 1, -1).astype(np.int64)
    B, n_plus = phi.size, int((phi > 0).sum())
    w = phi * B - (2 * n_plus - B) if 0 < n_plus < B else phi
    return w.astype(np.int32), n_plus


def direction(w, z):
    """v = sum_j w_j z_j from 0.0 in ascending j, one rounded add per j, and S = ssq(v)"""
    z = np.asarray(z, np.float32)
    v = np.zeros(z.shape[1], np.float64)
    for j in range(z.shape[0]):
        v = v + np.float64(int(w[j])) * z[j].astype(np.float64)
    return v, ssq(v)


def step(x, v, S, xi, m):
    """y_m = clip(x + c_m v, -1, 1), c_m = S > 0 ? (xi 2^-m) / sqrt(S) : 0"""
    c = (np.float64(xi) * np.float64(2.0 ** -m)) / np.sqrt(np.float64(S)) if S > 0 else np.float64(0.0)
    return clip1(np.asarray(x, np.float64) + c * np.asarray(v, np.float64))


def adversarial(d, attack_type, label):
    if d == -2:
        return False
    return d == label if attack_type == "targeted" else d != label


def round_candidates(r, lo, hi, G):
    """-> (the candidates of round r on q, ascending; whether this is the last round by the d - 1 <= G rule)"""
    if r == 0:
        return [((j + 1) * Q) // G for j in range(G)], False
    d = hi - lo
    if d - 1 <= G:
        return list(range(lo + 1, hi)), True
    return [lo + ((j + 1) * d) // (G + 1) for j in range(G)], False


def bracket(ok, G, max_rounds, may_score=lambda r, rows: True):
    """the bracket on q: ok(qs) -> one flag per candidate.  -> (hi or -1, rounds scored, [(lo, hi) after every round])"""
    lo, hi, rounds, hist = 0, -1, 0, []
    for r in range(max_rounds):
        qs, last = round_candidates(r, lo, hi, G)
        if not may_score(r, len(qs)):
            break
        flags = [bool(f) for f in ok(qs)]
        rounds = r + 1
        good = [q for q, f in zip(qs, flags) if f]
        if good:
            hi = good[0]
            below = [q for q in qs if q < hi]
            if below:
                lo = below[-1]
        elif hi >= 0 and qs:
            lo = qs[-1]
        hist.append((lo, hi))
        if hi < 0 or hi - lo == 1 or last:
            break
    return hi, rounds, hist


def drive(a, init, params, attack_type, label, noise, seed, stream, max_iter, decisions=None, victim=None, bits=16):
    """A whole attack.  The scored rows' decisions come from the log `decisions` (in scoring order) or, decisions=None, from
    victim(rows int16 (R, N)) -> R decisions, and are logged.  -> dict(success, adv, x, dist2, n_iters, n_queries, trace
    (n_iters + 1, 8), xs (the x after the start and after every iteration), batches (every scored batch, int16),
    decisions (the log), adopted (the decision of every row that became adv))."""
    a, init = np.asarray(a, np.float64).reshape(-1), np.asarray(init, np.float64).reshape(-1)
    n, G, R = a.size, params["grid"], params["max_rounds"]
    log, batches, adopted = [], [], []
    state = dict(queries=0, stopped=False, best=None)

    def over(rows):
        return params["max_queries"] > 0 and state["queries"] + rows > params["max_queries"]

    def score(rows):
        rows = np.ascontiguousarray(rows, np.int16)
        if decisions is not None:
            d = [int(v) for v in decisions[state["queries"]:state["queries"] + rows.shape[0]]]
            assert len(d) == rows.shape[0], "the decision log ends before the attack does"
        else:
            d = [int(v) for v in victim(rows)]
        batches.append(rows)
        log.extend(d)
        state["queries"] += rows.shape[0]
        return d

    def search(y, first_exempt):
        got = {}

        def ok(qs):
            rows = np.stack([cast_i16(line(a, y, q), bits) for q in qs])
            d = score(rows)
            flags = [adversarial(v, attack_type, label) for v in d]
            if any(flags):
                j = flags.index(True)
                got["row"], got["d"] = rows[j].copy(), d[j]
            return flags

        def may(r, rows):
            if (r == 0 and first_exempt) or not over(rows):
                return True
            state["stopped"] = True
            return False
        hi, rounds, _hist = bracket(ok, G, R, may)
        if hi >= 0:
            state["best"] = got["row"]
            adopted.append(got["d"])
        return hi, rounds

    trace, xs = [], []
    hi, rounds = search(init, True)
    if hi < 0:
        trace.append([0.0, 0.0, 0.0, -1.0, -1.0, float(rounds), float(state["queries"]), 0.0])
        return dict(success=-1, adv=cast_i16(a, bits), x=a.copy(), dist2=0.0, n_iters=0, n_queries=state["queries"],
                    trace=np.array(trace), xs=[], batches=batches, decisions=log, adopted=adopted)
    x = line(a, init, hi)
    D2 = ssq(x - a)
    xs.append(x)
    trace.append([D2, 0.0, 0.0, -1.0, float(hi), float(rounds), float(state["queries"]), 0.0])
    n_iters = 0
    for t in range(1, max_iter + 1):
        if state["stopped"]:
            break
        dist = math.sqrt(D2)
        B = num_evals(params, t)
        if over(B):
            break
        sigma = sigma_of(params, dist, n)
        z = noise((int(seed) ^ KEY) & 0xFFFFFFFFFFFFFFFF, t, stream, n, B)
        d = score(probes(x, sigma, z, bits))
        w, n_plus = weights([adversarial(v, attack_type, label) for v in d])
        v, S = direction(w, z)
        if over(G):
            break
        xi = dist / math.sqrt(float(t))
        ys = [step(x, v, S, xi, m) for m in range(G)]
        d = score(np.stack([cast_i16(y, bits) for y in ys]))
        good = [m for m in range(G) if adversarial(d[m], attack_type, label)]
        m, hi, rounds = (good[0] if good else -1), -1, 0
        if m >= 0:
            hi, rounds = search(ys[m], False)
            if rounds == 0:
                break
            if hi >= 0:
                x = line(a, ys[m], hi)
                D2 = ssq(x - a)
        xs.append(x)
        trace.append([D2, float(B), float(n_plus), float(m), float(hi), float(rounds), float(state["queries"]), sigma])
        n_iters = t
    return dict(success=1, adv=state["best"], x=x, dist2=D2, n_iters=n_iters, n_queries=state["queries"],
                trace=np.array(trace), xs=xs, batches=batches, decisions=log, adopted=adopted)
