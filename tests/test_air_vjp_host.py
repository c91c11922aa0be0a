"""White-box gradients through the over-the-air channel: the host side (no GPU).  The numpy twin and the PyTorch restatement
of tests/air_vjp_ref.py -- the adjoint identity on the unsaturated linear part, exact in integers; the mask rule on a
hand-made case --, header text, exported symbols and signatures, AdaptivePGD's and IvectorPGD's marshalling on the stub
engines of tests/test_whitebox_host.py, and the driver's rules on the stub site, for every accepted and every still-refused
combination of flags.  tests/test_gpu_air_vjp.py compares the kernels with the restatement."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

from fakebob_amd import _native as N
from fakebob_amd.engine import Engine
from fakebob_amd.pgd import PGD, AdaptivePGD, IvectorPGD
from tests import air_channel_ref as A
from tests import air_vjp_ref as AV
from tests.test_whitebox_host import _Engine, _header, _main, site      # noqa: F401 (site is a fixture)


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("L,n", [(2, 17), (255, 4000), (256, 100), (512, 2049)])
def test_adjoint_identity_on_the_linear_part_is_exact(L, n):
    """<c, conv(x)> == <corr(c), x> in int64: the twin's correlation is the transpose of air_channel_ref's sums"""
    rng = np.random.default_rng(L + n)
    t = rng.integers(-32767, 32768, L).astype(np.int16)
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    c = rng.integers(-2 ** 20, 2 ** 20 + 1, n)
    lhs = int((c * A.conv_sums(x, t)).sum())
    rhs = int((AV.correlate(t, c, np.int64) * x.astype(np.int64)).sum())
    assert lhs == rhs
    # float64 on integers below 2^53 and the int64 path agree bit for bit, and 2^-14 is exact
    assert np.array_equal(AV.conv_t(t, c, None, np.int64), AV.conv_t(t, c.astype(np.float64)))
    assert np.array_equal(AV.conv_t(t, c, None, np.int64) * 2.0 ** 14, AV.correlate(t, c, np.int64).astype(np.float64))


def test_the_mask_rule_on_a_hand_made_case():
    t, x = AV.full_range_case(64)
    n = x.size
    sat = AV.sat_mask(x, t)
    o = x.astype(np.int64) + np.concatenate([[0], x[:-1].astype(np.int64)])
    assert np.array_equal(A.conv_sums(x, t), 16384 * o)
    want = (np.abs(o) > 32767).astype(np.uint8)      # +32767 + 32767 = 65534: saturated; +-: 0; the first sample alone: not
    assert np.array_equal(sat, want) and sat[0] == 0 and sat[1] == 0 and sat[9] == 1 and sat[10] == 1 and sat[11] == 0
    assert 0 < sat.sum() < n / 4
    # an output AT a rail that was not clipped passes: x = [32767], one tap of 16384 -> o = 32767, unsaturated
    assert AV.sat_mask(np.array([32767, -32768], np.int16), np.array([16384, 0], np.int16)).sum() == 0
    # the transpose: a unit cotangent on an unsaturated output i reaches inputs i and i - 1 with weight 1; on a saturated one, nothing
    for i in (1, 9):
        c = np.zeros(n, np.int64)
        c[i] = 1
        dx = AV.conv_t(t, c, sat, np.int64)
        want_dx = np.zeros(n)
        if not sat[i]:
            want_dx[[i - 1, i]] = 1.0
        assert np.array_equal(dx, want_dx)


def test_the_autograd_function_is_the_twin():
    t, x = AV.full_range_case(40)
    cot = np.random.default_rng(1).normal(size=x.size)
    dwav, out = AV.defence_vjp(x, t, [], None, None, cot)
    assert np.array_equal(out, A.convolve(x, t))
    assert np.array_equal(dwav, AV.conv_t(t, cot, AV.sat_mask(x, t)))
    y = AV.AirChannel.apply(torch.tensor(x.astype(np.float64), requires_grad=True), t)
    assert y.requires_grad and y.dtype == torch.float64
    # the bound of a float64 sum holds between the float64 and the long double twin
    b = AV.bound(t, cot)
    assert (np.abs(AV.conv_t(t, cot) - AV.conv_t(t, cot, None, np.longdouble).astype(np.float64)) <= b + 1e-300).all()


# ------------------------------------------------------------------------------------------------ the surface
def test_entry_points_are_declared_and_exported():
    pub, hooks = _header("fakebob_hip.h"), _header("fakebob_hip_test.h")
    assert re.search(r"int fb_set_wb_air\(fb_engine \*e, int on\);", pub)
    assert re.search(r"int fb_debug_air_conv_t\(fb_engine \*e, const int16_t \*taps /\*\[B\]\[L\]\*/, int B, int L, int64_t n,", hooks)
    assert re.search(r"int fb_debug_wb_air_route\(fb_engine \*e, int \*n_launches\);", hooks)
    for word in ("fb_set_wb_air", "kept across fb_load_*", "(y[i] + 8192) >> 14", "j ascending", "No floating-point atomics",
                 "AIR CHANNEL: refused unless fb_set_wb_air", "k_air_conv_t"):
        assert word in pub, word
    assert "the transpose of the drawn room response is not in this version" not in pub
    assert "#define FB_WB_ROUTE_N 9" in hooks
    lib = C.CDLL(N.LIB_PATH)
    for name in ("fb_set_wb_air", "fb_debug_air_conv_t", "fb_debug_air_conv_t_chunk", "fb_debug_wb_air_route"):
        assert name in N.EXPORTS
        getattr(lib, name)
    assert lib.fb_version() == 103 and N.ABI_VERSION == 101
    assert 0 < lib.fb_debug_air_conv_t_chunk() <= 4096 and lib.fb_debug_air_conv_t_chunk() % 256 == 0


def test_signatures():
    assert list(inspect.signature(Engine.set_wb_air).parameters) == ["self", "on"]
    assert list(inspect.signature(Engine.debug_air_conv_t).parameters) == ["self", "taps", "cot", "sat"]
    assert list(inspect.signature(Engine.debug_wb_air_route).parameters) == ["self"]
    assert "set_wb_air" in Engine.get_grad_wb_iter.__doc__
    ad, iv = inspect.signature(AdaptivePGD.__init__).parameters, inspect.signature(IvectorPGD.__init__).parameters
    assert list(ad)[:7] == ["self", "task", "attack_type", "model", "bpda", "eot_size", "air"] and ad["air"].default is False
    assert list(iv)[:6] == ["self", "task", "attack_type", "model", "bpda", "air"] and iv["air"].default is False
    assert "air" not in inspect.signature(PGD.__init__).parameters


class _AirEngine(_Engine):
    def __init__(self, S, kind="gmm"):
        _Engine.__init__(self, S)
        self.kind, self.switches = kind, []

    def set_wb_air(self, on):
        self.switches.append(("air", on))

    def set_wb_ivector(self, on):
        self.switches.append(("ivector", on))

    def set_wb_bpda(self, on):
        self.switches.append(("bpda", on))

    def set_eot(self, r):
        self.switches.append(("eot", r))

    def attack_wb(self, p, audio):
        self.calls.append(("key", p.seed, p.stream))
        return _Engine.attack_wb(self, p, audio)


class _AirModel(object):
    def __init__(self, task, S, kind="gmm"):
        self.task, self.engine = task, _AirEngine(S, kind)


def test_adaptive_pgd_sets_the_switch_and_keys_the_draws():
    m = _AirModel("OSI", 3)
    pg = AdaptivePGD("OSI", "targeted", m, bpda=True, eot_size=8, air=True, seed=7, max_iter=3, verbose=False)
    assert m.engine.switches == [("eot", 8), ("bpda", True), ("air", True)] and pg.air is True and pg.eot_size == 8
    pg._stream = 2
    adv, flag = pg.attack(np.linspace(-0.5, 0.5, 40), None, threshold=0.25, target=2)
    assert m.engine.calls[0] == ("key", 7, 2) and adv.shape == (40, 1)
    # the channel alone: no BPDA switch, no set_eot, and the seed still keys the rooms
    m = _AirModel("OSI", 3)
    pg = AdaptivePGD("OSI", "targeted", m, bpda=False, air=True, seed=7, max_iter=3, verbose=False)
    assert m.engine.switches == [("air", True)] and pg.bpda is False
    pg.attack(np.linspace(-0.5, 0.5, 40), None, threshold=0.25, target=2)
    assert m.engine.calls[0] == ("key", 7, 0)
    # without the keyword nothing new is called and nothing is keyed
    m = _AirModel("OSI", 3)
    pg = AdaptivePGD("OSI", "targeted", m, bpda=False, seed=7, max_iter=3, verbose=False)
    pg.attack(np.linspace(-0.5, 0.5, 40), None, threshold=0.25, target=2)
    assert m.engine.switches == [] and pg.air is False and m.engine.calls[0] == ("key", 0, 0)
    with pytest.raises(ValueError):
        AdaptivePGD("OSI", "targeted", _AirModel("OSI", 3), bpda=False, eot_size=2, air=True)      # EOT still needs BPDA


@pytest.mark.parametrize("kind", ["iv", "gmm"])
def test_ivector_pgd_sets_the_switch(kind):
    m = _AirModel("OSI", 3, kind)
    pg = IvectorPGD("OSI", "targeted", m, air=True, seed=7, max_iter=3, verbose=False)
    assert m.engine.switches == [("ivector", True), ("air", True)] and pg.air is True and pg.eot_size == 1
    pg.attack(np.linspace(-0.5, 0.5, 40), None, threshold=0.25, target=2)
    assert m.engine.calls[0] == ("key", 7, 0)
    m = _AirModel("OSI", 3, kind)
    IvectorPGD("OSI", "targeted", m, bpda=True, verbose=False)
    assert m.engine.switches == [("ivector", True), ("bpda", True)]


# ------------------------------------------------------------------------------------------------ attack_main
AIR = ["--air-channel", "t60:200-600"]
ACCEPTED = [
    (["--bpda", "--wb-air"] + AIR, dict(bpda=True, eot_size=1, air=True)),
    (["--bpda", "--wb-air", "--eot-size", "8"] + AIR, dict(bpda=True, eot_size=8, air=True)),
    (["--bpda", "--wb-air", "--input-transform", "ms:7", "--codec", "ulaw"] + AIR, dict(bpda=True, eot_size=1, air=True)),
    (["--bpda", "--wb-air"], dict(bpda=True, eot_size=1, air=True)),                       # the switch without a channel: harmless
    (["-archi", "iv", "--wb-ivector", "--wb-air"] + AIR, dict(air=True)),
    (["-archi", "iv", "--wb-ivector", "--bpda", "--wb-air", "--codec", "ulaw"] + AIR, dict(bpda=True, air=True)),
]
REFUSED = [
    (AIR, "--air-channel"),                                                    # today's texts, without the flag
    (["--bpda"] + AIR, "--air-channel"),
    (["-archi", "iv", "--wb-ivector"] + AIR, "--air-channel"),
    (["--wb-air"] + AIR, "--air-channel"),                                     # GMM-UBM: only under --bpda
    (["-archi", "iv", "--bpda", "--wb-air"] + AIR, "GMM-UBM systems only"),    # -archi iv: only under --wb-ivector
    (["--wb-air"], "--wb-air"),
    (["--bpda", "--wb-air", "--feco", "0.5"] + AIR, "--feco"),
    (["--bpda", "--wb-air", "--dither", "1.0"] + AIR, "--dither"),
    (["--bpda", "--wb-air", "--companions", "1"] + AIR, "companion"),
    (["-archi", "iv", "--wb-ivector", "--wb-air", "--eot-size", "2"] + AIR, "--eot-size"),
    (["-archi", "iv", "--wb-ivector", "--wb-air", "--input-transform", "ms:7"] + AIR, "--input-transform"),
]


@pytest.mark.parametrize("extra,want", ACCEPTED, ids=[" ".join(a[0]) for a in ACCEPTED])
def test_attack_main_accepts(site, extra, want):
    (g, results, _thr), seen = _main(["--attack", "pgd"] + extra)
    assert g[1] == len(results) > 0
    new = {k: v for k, v in seen[0].items() if k in ("bpda", "eot_size", "air")}
    assert new == want and "samples_per_draw" not in seen[0]


@pytest.mark.parametrize("extra,word", REFUSED, ids=[" ".join(a[0]) for a in REFUSED])
def test_attack_main_refuses_before_any_model_is_built(site, capsys, extra, word):
    built = []
    with pytest.raises(SystemExit):
        _main(["--attack", "pgd"] + extra, built)
    assert built == []


def test_attack_main_refusal_texts(site):
    """the error texts: today's without --wb-air, --bpda's pattern for the flag outside --attack pgd"""
    import contextlib
    import io
    from fakebob_amd import attack_main as AM

    def err_of(argv):
        err = io.StringIO()
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(err), pytest.raises(SystemExit):
            AM.main(["-spk_id", "a", "-task", "OSI", "-type", "targeted"] + argv, model_factory=lambda *a: None, bob_factory=lambda *a, **k: None)
        return err.getvalue()
    assert "--attack pgd attacks an undefended victim: --air-channel t60:200-600 is not differentiated in this version" in err_of(["--attack", "pgd", "--bpda"] + AIR)
    assert "--attack pgd attacks an undefended victim: --air-channel t60:200-600 is not differentiated in this version" in err_of(["--attack", "pgd"] + AIR)
    for attack in ([], ["--attack", "nes"], ["--attack", "pso"]):
        assert "--wb-air belongs to --attack pgd" in err_of(attack + ["--wb-air"])
    assert "--wb-air" in err_of(["--attack", "pgd", "--wb-air"])
