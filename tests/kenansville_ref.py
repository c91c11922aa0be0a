"""The "decision-only attack" section of include/fakebob_hip.h restated in plain Python integers, window by window and
bin by bin, with no numpy arithmetic and nothing imported from fakebob_amd: the independent side of every bit-for-bit
comparison (fakebob_amd/kenansville.py is the vectorised twin, the kernels are the third).  The search is a pure function
of a callback that says which candidates of a round succeed.  Test infrastructure, not part of the product."""
import math

import numpy as np


def tables(W):
    """CF, SF, CI, SI as lists of Python ints (round() rounds half to even, as rint does)"""
    c = [math.cos(2.0 * math.pi * j / W) for j in range(W)]
    s = [math.sin(2.0 * math.pi * j / W) for j in range(W)]
    return ([int(round(v * 2.0 ** 30)) for v in c], [int(round(v * 2.0 ** 30)) for v in s],
            [int(round(v * 2.0 ** 22)) for v in c], [int(round(v * 2.0 ** 22)) for v in s])


def weight(k, W):
    return 1 if k == 0 or (W % 2 == 0 and k == W // 2) else 2


def analyse_window(xw, W, tab):
    """one window of W Python ints -> dict(A, B, a, b, p, cum, E, order)"""
    CF, SF = tab[0], tab[1]
    K = W // 2 + 1
    A, B = [], []
    for k in range(K):
        sa = sb = 0
        for n in range(W):
            j = (n * k) % W
            sa += xw[n] * CF[j]
            sb += xw[n] * SF[j]
        A.append(sa)
        B.append(sb)
    a = [(v + (1 << 29)) >> 30 for v in A]           # Python's >> floors, as an arithmetic shift does
    b = [(v + (1 << 29)) >> 30 for v in B]
    p = [a[k] * a[k] + b[k] * b[k] for k in range(K)]
    e = [weight(k, W) * p[k] for k in range(K)]
    order = sorted(range(K), key=lambda k: (p[k], k))
    cum, run = [0] * K, 0
    for k in order:
        run += e[k]
        cum[k] = run
    return dict(A=A, B=B, a=a, b=b, p=p, cum=cum, E=sum(e), order=order)


def analyse(x, W, tab=None):
    """-> (the zero-padded windows as lists of ints, one analyse_window dict per window)"""
    tab = tab or tables(W)
    xs = [int(v) for v in np.asarray(x).reshape(-1)]
    nw = -(-len(xs) // W)
    xs += [0] * (nw * W - len(xs))
    wins = [xs[w * W:(w + 1) * W] for w in range(nw)]
    return wins, [analyse_window(xw, W, tab) for xw in wins]


def threshold(E, q):
    return (E >> 16) * q + (((E & 0xFFFF) * q) >> 16)


def removed_bins(an, q):
    thr = threshold(an["E"], q)
    return [k for k in range(len(an["cum"])) if an["cum"][k] <= thr]


def candidate(n_samples, W, wins, ans, q, tab, stats=None):
    """candidate q from an analysis -> int16 array; stats (a dict) collects the largest sum of |terms of R|"""
    CI, SI = tab[2], tab[3]
    D = W << 22
    y = []
    for xw, an in zip(wins, ans):
        rem = removed_bins(an, q)
        for n in range(W):
            R = mag = 0
            for k in rem:
                j = (n * k) % W
                t1, t2 = weight(k, W) * an["a"][k] * CI[j], weight(k, W) * an["b"][k] * SI[j]
                R += t1 + t2
                mag += abs(t1) + abs(t2)
            if stats is not None:
                stats["R_mag"] = max(stats.get("R_mag", 0), mag)
            r = (2 * R + D) // (2 * D)                # Python's // floors
            y.append(min(max(xw[n] - r, -32768), 32767))
    return np.array(y[:n_samples], dtype=np.int16)


def remove(x, W, q, tab=None, stats=None):
    tab = tab or tables(W)
    wins, ans = analyse(x, W, tab)
    return candidate(np.asarray(x).size, W, wins, ans, int(q), tab, stats)


def candidates(x, W, qs, tab=None):
    """the analysis once, then every q of qs -> (len(qs), N) int16"""
    tab = tab or tables(W)
    wins, ans = analyse(x, W, tab)
    return np.stack([candidate(np.asarray(x).size, W, wins, ans, int(q), tab) for q in qs])


# ---------------------------------------------------------------------------------------------------- decisions
def decide(task, scores, threshold_, tv=1):
    """the system classes' make_decisions rule on one row of system scores; -2 for a row without voiced frames"""
    if tv <= 0:
        return -2
    s = [float(v) for v in np.asarray(scores).reshape(-1)]
    if task == "SV":
        return 1 if s[0] >= threshold_ else -1
    am = 0
    for m in range(1, len(s)):
        if s[m] > s[am]:
            am = m
    if task == "OSI" and s[am] < threshold_:
        return -1
    return am


def succeeds(d, attack_type, label):
    if d == -2:
        return False
    return d == label if attack_type == "targeted" else d != label


# ---------------------------------------------------------------------------------------------------- the search
def round_candidates(r, lo, hi, G, q_max):
    """-> (the candidates of round r, ascending; whether this is the last round by the d - 1 <= G rule)"""
    if r == 0:
        out = []
        for j in range(G):
            q = ((j + 1) * q_max) // G
            if q > 0 and (not out or q != out[-1]):
                out.append(q)
        return out, False
    d = hi - lo
    if d - 1 <= G:
        return list(range(lo + 1, hi)), True
    return [lo + ((j + 1) * d) // (G + 1) for j in range(G)], False


def search(ok, G, q_max, max_rounds):
    """ok(r, qs) -> one truth value per candidate: whether it succeeds.  -> dict(success, factor, n_queries, rounds), rounds
    a list of dict(qs, flags, lo, hi, rows, last) with lo / hi as they stand AFTER the round (hi None: none yet)."""
    lo, hi, queries, rounds = 0, None, 0, []
    for r in range(max_rounds):
        qs, last = round_candidates(r, lo, hi, G, q_max)
        flags = [bool(f) for f in ok(r, list(qs))]
        assert len(flags) == len(qs)
        queries += len(qs)
        good = [q for q, f in zip(qs, flags) if f]
        if good:
            hi = good[0]
            below = [q for q in qs if q < hi]
            if below:
                lo = below[-1]
        elif hi is not None and qs:
            lo = qs[-1]
        rounds.append(dict(qs=qs, flags=flags, lo=lo, hi=hi, rows=len(qs), last=last))
        if hi is None or hi - lo == 1 or last:
            break
    return dict(success=1 if hi is not None else -1, factor=-1 if hi is None else hi, n_queries=queries, rounds=rounds)


# ---------------------------------------------------------------------------------------------------- test signals
def edge_audio(W, N, seed=7):
    """int16 samples whose windows of W cycle through: synthetic speech, silence, a constant, constant -32768, full scale with
    alternating signs, a lone impulse at n = 0 (every p[k] equal: the (p, k) tie rule decides the order), speech again"""
    rng = np.random.RandomState(seed + 131 * W)
    nw = -(-N // W)
    t = np.arange(W)
    out = []
    for w in range(nw):
        kind = w % 7
        if kind in (0, 6):
            v = 6000.0 * np.sin(2 * np.pi * (2.3 + w) * t / W + w) + 2500.0 * np.sin(2 * np.pi * 0.31 * t + 1.0) + rng.normal(0, 300.0, W)
        elif kind == 1:
            v = np.zeros(W)
        elif kind == 2:
            v = np.full(W, 1234.0)
        elif kind == 3:
            v = np.full(W, -32768.0)
        elif kind == 4:
            v = np.where(t % 2 == 0, -32768.0, 32767.0)
        else:
            v = np.zeros(W)
            v[0] = 20000.0
        out.append(np.clip(np.rint(v), -32768, 32767))
    return np.concatenate(out)[:N].astype(np.int16)
