"""x-vector systems without a GPU: the PyTorch restatement of the contract (tests/xvector_ref.py) against a plain-loop
numpy one, fb_load_xvector's host images (fb_debug_prepare_xvector) against numpy, models.XvectorSystem's constructor and
npz round trip, and the refusals the host preparation gives by name."""
import numpy as np
import pytest
import torch

from fakebob_amd import _native as N
from fakebob_amd import prepare
from fakebob_amd.models import STOCK_XV_CONTEXTS, XvectorSystem, synthetic_xvector_system
from tests import xvector_ref as ref

D = 24


def small_system(**kw):
    args = dict(hidden=64, pool=96, R=64, L=32, n_speakers=3, seed=11)
    args.update(kw)
    return synthetic_xvector_system(D, **args)


def loop_stages(system, x):
    """the contract in plain loops, float64"""
    h = np.asarray(x, np.float32).astype(np.float64)
    T = h.shape[0]
    outs = []
    for ly in system.layers:
        W = ly["W"].astype(np.float64)
        din = h.shape[1]
        y = np.empty((T, W.shape[0]))
        for t in range(T):
            sp = np.empty(len(ly["ctx"]) * din)
            for j, c in enumerate(ly["ctx"]):
                sp[j * din:(j + 1) * din] = h[min(max(t + c, 0), T - 1)]
            for o in range(W.shape[0]):
                a = float(W[o] @ sp) + float(ly["bias"][o])
                y[t, o] = float(ly["bn_scale"][o]) * max(a, 0.0) + float(ly["bn_offset"][o])
        outs.append(y)
        h = y
    P = h.shape[1]
    st = np.empty(2 * P)
    for c in range(P):
        m = sum(h[t, c] for t in range(T)) / T
        v = sum(h[t, c] * h[t, c] for t in range(T)) / T - m * m
        st[c], st[P + c] = m, np.sqrt(max(v, 1e-10))
    emb = system.seg_W.astype(np.float64) @ st + system.seg_bias.astype(np.float64)
    return outs, st, emb


@pytest.mark.parametrize("T", [1, 2, 5])
def test_ref_against_plain_loops(T):
    sy = small_system()
    x = np.random.default_rng(T).normal(size=(T, D)).astype(np.float32)
    o1, s1, e1 = ref.stages(sy, x)
    o2, s2, e2 = loop_stages(sy, x)
    for a, b in zip(o1, o2):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert np.abs(s1 - s2).max() <= 1e-12 * max(1.0, np.abs(s2).max())
    assert np.abs(e1 - e2).max() <= 1e-12 * max(1.0, np.abs(e2).max())
    if T == 1:   # one row: every context place is that row, the variance is zero and the floor gives 1e-5
        P = sy.P
        assert np.all(s1[P:] == np.sqrt(1e-10))
    o32, s32, e32 = ref.stages(sy, x, torch.float32)
    assert np.abs(e32 - e1).max() <= 1e-4 * np.abs(e1).max()


def test_clamp_replicates_the_utterances_own_edges():
    assert ref.splice_index(3, (-2, 0, 2)).tolist() == [[0, 0, 2], [0, 1, 2], [0, 2, 2]]
    assert ref.splice_index(1, (-3, 0, 3)).tolist() == [[0, 0, 0]]


@pytest.mark.parametrize("l", [0, 1, 4])
def test_weight_images_against_numpy(l):
    sy = small_system(pool=100)          # the last layer's fourth column tile is partial
    img = prepare.xvector_buffer(sy, "w%d" % l)
    kw = int(prepare.xvector_buffer(sy, "kw")[l])
    W = sy.layers[l]["W"]
    dout, K = W.shape
    amax = float(np.abs(W).max())
    assert 2.0 ** 14 <= amax * 2.0 ** -kw < 2.0 ** 15
    n_steps = (K + 15) // 16
    tiles = (dout + 31) // 32
    assert img.size == tiles * n_steps * 2 * 64 * 8
    img = img.reshape(tiles, n_steps, 2, 2, 32, 8)            # tile, step, term, K half, channel place, place
    Wp = np.zeros((tiles * 32, n_steps * 16), np.float32)     # zeros past K and past dout
    Wp[:dout, :K] = np.ldexp(W, -kw)
    hi = Wp.astype(np.float16)
    lo = (Wp - hi.astype(np.float32)).astype(np.float16)
    for term, part in ((0, hi), (1, lo)):
        want = part.view(np.uint16).reshape(tiles, 32, n_steps, 2, 8).transpose(0, 2, 3, 1, 4)
        assert np.array_equal(img[:, :, term], want), term
    # the two terms carry the weight to 22 bits
    back = np.ldexp(hi.astype(np.float64) + lo.astype(np.float64), kw)[:dout, :K]
    assert np.abs(back - W).max() <= 2.0 ** -22 * amax


def test_segment_and_backend_tables():
    sy = small_system()
    segT = prepare.xvector_buffer(sy, "segT").reshape(2 * sy.P, sy.R)
    assert np.array_equal(segT, sy.seg_W.astype(np.float64).T)
    be = prepare.xvector_buffer(sy, "backend")
    off = prepare.xvector_buffer(sy, "backend_offsets")
    L, S = sy.L, sy.S
    tr = be[off[5]:off[5] + S * L].reshape(S, L)
    want = np.stack([ref.backend_transform(sy, e) for e in sy.enrolled])
    assert np.abs(tr - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(be[off[1]:off[1] + sy.R * L].reshape(sy.R, L), sy.lda.astype(np.float64).T)


def test_constructor_and_npz_round_trip(tmp_path):
    sy = small_system()
    assert [ly["ctx"] for ly in sy.layers] == [tuple(c) for c in STOCK_XV_CONTEXTS]
    assert [ly["W"].shape for ly in sy.layers] == [(64, 5 * D), (64, 192), (64, 192), (64, 64), (96, 64)]
    assert (sy.P, sy.R, sy.L, sy.S) == (96, 64, 32, 3) and sy.seg_W.shape == (64, 192)
    assert all(ly["W"].dtype == np.float32 for ly in sy.layers) and sy.plda_psi.dtype == np.float64
    p = str(tmp_path / "xvector.npz")
    sy.save(p)
    sy2 = XvectorSystem.load(p)
    a, b = sy.to_arrays(), sy2.to_arrays()
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    sy3 = sy.with_enrolled(np.ones((2, sy.R)), [0.5, 1.0], [2.0, 3.0])
    assert sy3.S == 2 and sy3.z_std.tolist() == [2.0, 3.0] and sy3.layers[0]["W"] is sy.layers[0]["W"]
    with pytest.raises(AssertionError):
        XvectorSystem(D, [dict(sy.layers[0], W=np.zeros((64, 7)))], sy.seg_W, sy.seg_bias, sy.mean_vec, sy.lda, sy.plda_mean,
                      sy.plda_transform, sy.plda_psi, sy.enrolled)
    # He-scaled: a unit-variance input neither dies nor blows up on its way through the five layers
    x = np.random.default_rng(0).normal(size=(40, D)).astype(np.float32)
    outs, _, emb = ref.stages(sy, x)
    for o in outs:
        assert 0.1 < o.std() < 10.0
    assert np.all(np.isfinite(emb))


def _refused(sy, text):
    with pytest.raises(N.NativeError) as ei:
        prepare.xvector_buffer(sy, "kw")
    assert ei.value.code == N.FB_E_ARG and text in str(ei.value), str(ei.value)


def test_limits_are_refused_by_name():
    _refused(small_system(R=48, L=16), "R=48 must be a multiple of 32")
    _refused(small_system(n_speakers=61), "at most 60 enrolled speakers")
    _refused(small_system(pool=2049), "dout=2049 outside 1 .. 2048")
    _refused(synthetic_xvector_system(D, 64, 96, 64, 32, contexts=((-3, -2, -1, 0, 1, 2), (0,))), "n_ctx=6 outside 1 .. 5")
    _refused(synthetic_xvector_system(D, 64, 96, 64, 32, contexts=((0, -1), (0,))), "context offsets must ascend")
    _refused(synthetic_xvector_system(D, 64, 96, 64, 32, contexts=((-9, 0), (0,))), "context offset -9 outside -8 .. 8")
    with pytest.raises(ValueError):      # (the struct has no room for a ninth layer: refused before the library sees it)
        prepare.xvector_buffer(synthetic_xvector_system(D, 64, 96, 64, 32, contexts=((0,),) * 9), "kw")
    with pytest.raises(N.NativeError) as ei:
        prepare.xvector_buffer(small_system(), "w7")
    assert "no x-vector buffer" in str(ei.value)
