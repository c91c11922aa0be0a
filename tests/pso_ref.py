"""numpy restatement of the particle-swarm attack (fb_attack_pso), written from the "particle-swarm attack" section of
include/fakebob_hip.h and nothing else: the uniforms, the initialisation, one update, and `replay` -- the whole state machine
driven by a given table of losses.  `philox(counter[4], key[2]) -> 4 words` is handed in (oracle.philox), so this module
needs no library.  Every line below is one float64 operation of the contract: numpy rounds each to nearest and fuses none."""
import numpy as np

PSWM = 0x5053574D
M32 = 0xFFFFFFFF


def U(w):
    """((double)w + 0.5) * 2^-32"""
    return (np.asarray(w, np.float64) + 0.5) * 2.0 ** -32


def clip(s, l, h):
    return np.minimum(np.maximum(s, l), h)


def cast_i16(x, bits=16):
    """the engine's int16 cast: trunc(x * 2^(bits - 1)), low 16 bits"""
    return np.trunc(np.asarray(x, np.float64) * 2.0 ** (bits - 1)).astype(np.int64).astype(np.int16)


def ball(a, eps):
    a = np.asarray(a, np.float64)
    return clip(a - eps, -1.0, 1.0), clip(a + eps, -1.0, 1.0)


_cache = {}


def uniforms(philox, seed, stream, t, P, n):
    """(first, second) uniforms [P][n] of update t (t = 0: the initialisation): words 0, 1 of counter (i >> 1, p, t, 0) serve
    element 2 (i >> 1), words 2, 3 element 2 (i >> 1) + 1; of a pair the first word is u_x / r1, the second u_v / r2."""
    k = (seed, stream, t, P, n)
    if k not in _cache:
        key = [(seed & M32) ^ PSWM, ((seed >> 32) & M32) ^ (stream & M32)]
        w = np.zeros((P, 2 * ((n + 1) // 2), 2), np.float64)
        for p in range(P):
            for j in range((n + 1) // 2):
                o = philox([j, p, t & M32, 0], key)
                w[p, 2 * j] = o[0], o[1]
                w[p, 2 * j + 1] = o[2], o[3]
        if len(_cache) > 64:
            _cache.clear()
        _cache[k] = (U(w[:, :n, 0]), U(w[:, :n, 1]))
    return _cache[k]


def init(philox, a, eps, P, v_max, seed, stream, bits=16):
    """-> x, v [P][n], q = the first batch"""
    a = np.asarray(a, np.float64)
    lo, hi = ball(a, eps)
    ux, uv = uniforms(philox, seed, stream, 0, P, a.size)
    d = hi - lo
    m = ux * d
    x = clip(lo + m, lo, hi)
    v = (2.0 * uv - 1.0) * v_max
    x[0] = a
    v[0] = 0.0
    return x, v, cast_i16(x, bits)


def step(philox, a, eps, x, v, pb, gb, improved, g_new, w, c1, c2, v_max, seed, stream, t, bits=16):
    """the move `t` with the host's decisions riding along: pb_p = x_p where improved[p], gb = x[g_new] unless g_new = -1,
    both before the velocities read them -> x', v', pb', gb', q'"""
    a = np.asarray(a, np.float64)
    x, v, pb, gb = (np.array(z, np.float64) for z in (x, v, pb, gb))
    P = x.shape[0]
    lo, hi = ball(a, eps)
    imp = np.asarray(improved).astype(bool)
    pb[imp] = x[imp]
    if g_new >= 0:
        gb = x[g_new].copy()
    r1, r2 = uniforms(philox, seed, stream, t, P, a.size)
    inert = w * v
    cog = (c1 * r1) * (pb - x)
    soc = (c2 * r2) * (gb - x)
    vn = clip((inert + cog) + soc, -v_max, v_max)
    xn = clip(x + vn, lo, hi)
    return xn, vn, pb, gb, cast_i16(xn, bits)


def replay(philox, a, losses, eps, max_iter, P, w_init, w_end, c1, c2, v_max, seed, stream, bits=16, scores=None, keep=()):
    """The attack driven by losses[k][p] (rows are consumed until it stops; it stops at the last row at the latest, which
    must then be row max_iter - 1 or a stopping one) -- or by a scorer losses(k, x [P][n]) -> the P losses of iteration k.
    scores (optional) [k][p][S]: what gs is taken from.
    -> dict(n_iters, success, trace rows [gl, g, improved (, gs)], adv_f64, adv_i16, gl, positions {k: x of iteration k for k in keep})"""
    a = np.asarray(a, np.float64)
    if not callable(losses):
        losses = np.asarray(losses, np.float64)
    x, v, _q = init(philox, a, eps, P, v_max, seed, stream, bits)
    pb, gb = x.copy(), x[0].copy()
    pl = np.zeros(P)
    gl, g, gs = 0.0, 0, None
    trace, positions = [], {}
    k = 0
    while True:
        if k in keep:
            positions[k] = x.copy()
        l = np.asarray(losses(k, x), np.float64) if callable(losses) else losses[k]
        imp = np.ones(P, bool) if k == 0 else l < pl
        pl = np.where(imp, l, pl)
        pb[imp] = x[imp]
        gstar = int(np.argmin(pl))                      # the lowest p among the minimal ones
        g_new = -1
        if k == 0 or pl[gstar] < gl:
            gl, g, g_new = float(pl[gstar]), gstar, gstar
            gb = pb[gstar].copy()
            if scores is not None:
                gs = np.array(scores[k][gstar], np.float64).reshape(-1)
        trace.append([gl, float(g), float(imp.sum())] + ([] if gs is None else list(gs)))
        if gl < 0:
            success = 1
            break
        if k == max_iter - 1:
            success = -1
            break
        w_k = w_init - ((w_init - w_end) * float(k)) / float(max_iter)
        x, v, pb, gb, _q = step(philox, a, eps, x, v, pb, gb, imp, g_new, w_k, c1, c2, v_max, seed, stream, k + 1, bits)
        k += 1
    return dict(n_iters=k + 1, success=success, trace=np.array(trace), adv_f64=gb, adv_i16=cast_i16(gb, bits), gl=gl,
                positions=positions)
