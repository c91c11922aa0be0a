"""The numpy float64 host twin of fb_attack_cw2 (the "CW2" contract of include/fakebob_hip.h): the block-ordered L2, one
iteration's control decisions and Adam step, the rule that moves the constant between search steps, and a whole attack
replayed on gradients from Engine.get_grad_wb_iter.  Every expression is written as the contract's pseudo-code writes it, so
numpy rounds where the device rounds; tanh is the one function the two do not share bit for bit."""
import math

import numpy as np


def cast_i16(x, bits=16):
    """the forward's int16 cast of float audio: truncation of x * 2^(bits - 1), wrapped to 16 bits"""
    v = np.trunc(np.asarray(x, np.float64) * float(2 ** (bits - 1))).astype(np.int64)
    return (v & 0xFFFF).astype(np.uint16).view(np.int16)


def w0_of(a0):
    """atanh(0.999999 a0) by the C library's atanh, element by element (math.atanh calls it; numpy's vector loops may not)"""
    return np.array([math.atanh(0.999999 * float(v)) for v in np.asarray(a0, np.float64)], np.float64)


def l2_blocks(x, a0):
    """sum (x - a0)^2 in the contract's order: blocks of 256 consecutive samples padded with +0.0, within a block
    d[i] += d[i + h] for h = 128, 64, ..., 1, then the partials in ascending block order from +0.0"""
    d = np.asarray(x, np.float64) - np.asarray(a0, np.float64)
    d = d * d
    nb = (d.size + 255) // 256
    v = np.zeros(nb * 256, np.float64)
    v[:d.size] = d
    v = v.reshape(nb, 256)
    h = 128
    while h >= 1:
        v = v[:, :h] + v[:, h:2 * h]
        h //= 2
    total = 0.0
    for b in range(nb):
        total = total + float(v[b, 0])
    return total


def control(adver_loss, l2, c, gbest_l2, t, prev, abort_every):
    """k_cw2_ctl's decisions -> dict(gate, take, found, gbest_l2, L, abort, prev)"""
    gate = 1 if adver_loss > 0 else 0
    L = (c * gate) * adver_loss + l2
    take = bool(adver_loss < 0 and l2 < gbest_l2)
    abort = False
    if abort_every > 0 and t % abort_every == 0:
        if L > 0.9999 * prev:
            abort = True
        else:
            prev = L
    return dict(gate=gate, take=int(take), found=bool(adver_loss < 0), gbest_l2=l2 if take else gbest_l2, L=L, abort=abort, prev=prev)


def adam_step(g, x, a0, w0, mod, m1, m2, c, gate, p1, p2, lr=1e-2, beta1=0.9, beta2=0.999, adam_eps=1e-8):
    """k_cw2_step's update; p1 = beta1^(t+1), p2 = beta2^(t+1) by repeated multiplication -> (mod, m1, m2, x_next)"""
    G = ((c * gate) * g + 2.0 * (x - a0)) * (1.0 - x * x)
    m1 = beta1 * m1 + (1.0 - beta1) * G
    m2 = beta2 * m2 + ((1.0 - beta2) * G) * G
    mod = mod - ((lr / (1.0 - p1)) * m1) / (np.sqrt(m2) / math.sqrt(1.0 - p2) + adam_eps)
    return mod, m1, m2, np.tanh(w0 + mod)


def next_const(found, lo, hi, c):
    """the search-constant rule between two search steps -> (lo, hi, c)"""
    if found:
        hi = min(hi, c)
        c = (lo + hi) / 2.0
    else:
        lo = max(lo, c)
        c = (lo + hi) / 2.0 if hi < 1e9 else c * 10.0
    return lo, hi, c


def const_sequence(initial_const, founds):
    """the constants of the search steps whose outcomes are `founds`, and the one after the last"""
    lo, hi, c, out = 0.0, 1e10, float(initial_const), []
    for f in founds:
        out.append(c)
        lo, hi, c = next_const(f, lo, hi, c)
    return out, c


def replay(eng, p, q, audio):
    """fb_attack_cw2 on the host: the contract's pseudo-code, the gradient from Engine.get_grad_wb_iter(p, x, epoch) at every
    iterate -> dict like Engine.attack_cw2's, plus min_margin: the smallest distance, in LSB, of a sample of any iterate from an
    int16 rounding boundary (a case is usable only when no device / host tanh difference can move a cast)"""
    a0 = np.asarray(audio, np.float64).reshape(-1)
    bits = p.bits_per_sample or 16
    w0 = w0_of(a0)
    c, lo, hi = q.initial_const, 0.0, 1e10
    gbest_l2, gbest_row, gbest_x = float("inf"), cast_i16(a0, bits), a0.copy()
    rows, per, margin = [], [], float("inf")
    for s in range(q.search_steps):
        mod, m1, m2 = np.zeros_like(a0), np.zeros_like(a0), np.zeros_like(a0)
        x = np.tanh(w0)
        p1 = p2 = 1.0
        prev, found, n_rows = float("inf"), False, 0
        for t in range(p.max_iter):
            epoch = s * p.max_iter + t
            scaled = x * float(2 ** (bits - 1))
            near = np.round(scaled)   # (truncation: the boundaries are the non-zero integers)
            margin = min(margin, float(np.min(np.where(near == 0.0, 1.0 - np.abs(scaled), np.abs(scaled - near)))))
            g, al, sc = eng.get_grad_wb_iter(p, x, epoch)
            l2 = l2_blocks(x, a0)
            d = control(al, l2, c, gbest_l2, t, prev, q.abort_every)
            rows.append([l2, al, c] + list(sc))
            n_rows += 1
            if d["take"]:
                gbest_l2, gbest_row, gbest_x = l2, cast_i16(x, bits), x.copy()
            found = found or d["found"]
            prev = d["prev"]
            if d["abort"]:
                break
            p1 *= q.beta1
            p2 *= q.beta2
            mod, m1, m2, x = adam_step(g, x, a0, w0, mod, m1, m2, c, d["gate"], p1, p2, q.lr, q.beta1, q.beta2, q.adam_eps)
        per.append(n_rows)
        lo, hi, c = next_const(found, lo, hi, c)
    return dict(adv=gbest_row, success=1 if gbest_l2 < float("inf") else -1, adver_f64=gbest_x, trace=np.array(rows),
                rows_per_step=np.array(per, np.int32), best_l2=gbest_l2, const=c, min_margin=margin)
