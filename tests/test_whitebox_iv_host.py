"""White-box gradients through the i-vector-PLDA victim: the host side.  No GPU: header text, exported symbols, signatures,
IvectorPGD's marshalling on a stub engine, and the driver's rules on the stub site of tests/golden/driver_site.py."""
import ctypes as C
import inspect
import pickle
import re

import numpy as np
import pytest

from fakebob_amd import _native as N
from fakebob_amd.engine import Engine
from fakebob_amd.pgd import PGD, AdaptivePGD, IvectorPGD
from tests.test_whitebox_host import _Engine, _header, _main, _Model, site      # noqa: F401 (site is a fixture)


def test_entry_points_are_declared_and_exported():
    pub, hooks = _header("fakebob_hip.h"), _header("fakebob_hip_test.h")
    assert re.search(r"int fb_set_wb_ivector\(fb_engine \*e, int on\);", pub)
    assert re.search(r"int fb_debug_iv_backend_grad\(fb_engine \*e, const double \*ivec /\*\[R\]\*/, const double \*w /\*\[S\]\*/, "
                     r"double \*out /\*\[R\]\*/\);", hooks)
    assert re.search(r"int fb_debug_iv_feat_grad\(fb_engine \*e, const float \*feats, int Tv, const double \*cot /\*\[R\]\*/, "
                     r"double \*out /\*\[Tv\*D\]\*/\);", hooks)
    for word in ("fb_set_wb_ivector", "gmm-gselect is a constant", "--min-post pruning is a constant set", "constant posterior",
                 "quad^-1 wbar", "k_wb_iv_backend_t", "k_wb_iv_stats_t", "k_wb_iv_post_t", "Nbar_k = - lambda' U_k w",
                 "one row's i-vector state", "not positive definite"):
        assert word in pub, word
    for word in ("FB_WB_ROUTE_IV_CTL 4", "FB_WB_ROUTE_IV_POST_T 8", "FB_WB_ROUTE_N 9"):
        assert word in hooks, word
    # the indices the existing counters had keep their meaning
    for word in ("FB_WB_ROUTE_CTL 0", "FB_WB_ROUTE_CTL_REP 1", "FB_WB_ROUTE_BACKWARD 2", "FB_WB_ROUTE_CHAIN_T 3"):
        assert word in hooks, word
    lib = C.CDLL(N.LIB_PATH)
    for name in ("fb_set_wb_ivector", "fb_debug_iv_backend_grad", "fb_debug_iv_feat_grad"):
        assert name in N.EXPORTS
        getattr(lib, name)
    assert lib.fb_version() >= 102


def test_engine_signatures():
    assert list(inspect.signature(Engine.set_wb_ivector).parameters) == ["self", "on"]
    assert list(inspect.signature(Engine.debug_iv_backend_grad).parameters) == ["self", "ivec", "w"]
    assert list(inspect.signature(Engine.debug_iv_feat_grad).parameters) == ["self", "feats", "cot"]
    assert "set_wb_ivector" in Engine.get_grad_wb_iter.__doc__ and "set_wb_ivector" in Engine.attack_wb.__doc__
    pg, iv = inspect.signature(PGD.__init__).parameters, inspect.signature(IvectorPGD.__init__).parameters
    assert list(iv)[:5] == ["self", "task", "attack_type", "model", "bpda"] and iv["bpda"].default is False
    assert list(inspect.signature(AdaptivePGD.__init__).parameters)[:6] == ["self", "task", "attack_type", "model", "bpda", "eot_size"]
    assert "adver_thresh" in pg and PGD.KINDS == ("gmm",) and IvectorPGD.KINDS == ("gmm", "iv")
    for name in ("attack", "get_grad", "estimate_threshold", "_params"):
        assert getattr(IvectorPGD, name) is getattr(PGD, name)


class _IvEngine(_Engine):
    def __init__(self, S, kind):
        _Engine.__init__(self, S)
        self.kind, self.switches = kind, []

    def set_wb_ivector(self, on):
        self.switches.append(("ivector", on))

    def set_wb_bpda(self, on):
        self.switches.append(("bpda", on))

    def set_eot(self, r):
        self.switches.append(("eot", r))


class _IvModel(object):
    def __init__(self, task, S, kind):
        self.task, self.engine = task, _IvEngine(S, kind)


@pytest.mark.parametrize("kind", ["iv", "gmm"])
@pytest.mark.parametrize("bpda", [False, True])
def test_ivector_pgd_sets_the_switch_and_marshals_as_pgd(tmp_path, kind, bpda):
    m = _IvModel("OSI", 3, kind)
    pg = IvectorPGD("OSI", "targeted", m, bpda=bpda, adver_thresh=0.5, epsilon=0.003, max_iter=9, max_lr=2e-3, min_lr=1e-5,
                    momentum=0.0, plateau_length=4, plateau_drop=3.0, seed=7, verbose=False)
    assert m.engine.switches == [("ivector", True)] + ([("bpda", True)] if bpda else [])      # never set_eot
    assert pg.bpda is bpda and pg.eot_size == 1
    cp = str(tmp_path / "a.cp")
    adv, flag = pg.attack(np.linspace(-0.5, 0.5, 40), cp, threshold=0.25, target=2, bits_per_sample=12)
    assert adv.dtype == np.int16 and adv.shape == (40, 1) and flag == 1
    assert m.engine.calls == [("wb", 0, 9, 0.003, 2e-3, 1e-5, 0.0, 4, 3.0, 0.25, 2, 0, 0.5, 12)]
    with open(cp, "rb") as r:
        rows = pickle.load(r)
    assert len(rows) == 3 and all(len(row) == 4 and row[1].shape == (1,) and row[2].shape == (3,) for row in rows)
    assert pg._params().seed == (7 if bpda else 0)      # the seed keys a defended victim's draws only
    g, al, sc = pg.get_grad(np.zeros(40))
    assert g.shape == (40, 1) and al.shape == (1,) and sc.shape == (3,)


def test_pgd_and_adaptive_pgd_still_refuse_an_ivector_engine():
    for cls, kw in ((PGD, {}), (AdaptivePGD, dict(bpda=True)), (AdaptivePGD, dict(bpda=False))):
        m = _IvModel("OSI", 3, "iv")
        with pytest.raises(ValueError) as ex:
            cls("OSI", "targeted", m, **kw)
        assert "i-vector" in str(ex.value) and m.engine.switches == []
    with pytest.raises(TypeError):
        IvectorPGD("OSI", "targeted", object())
    with pytest.raises(ValueError):
        IvectorPGD("SV", "targeted", _IvModel("OSI", 3, "iv"))
    m = _Model("OSI", 3)
    m.engine.kind = "foreign"
    m.engine.set_wb_ivector = lambda on: None
    with pytest.raises(ValueError):
        IvectorPGD("OSI", "targeted", m)


# ------------------------------------------------------------------------------------------------ attack_main
def test_attack_main_builds_for_archi_iv_with_the_switch(site):
    built = []
    (g, results, _thr), seen = _main(["--attack", "pgd", "-archi", "iv", "--wb-ivector", "-max_iter", "40"], built)
    assert len(built) == 1 and "iv-OSI-targeted" in built[0]
    assert seen == [dict(adver_thresh=0.0, epsilon=0.002, max_iter=40, max_lr=0.001, min_lr=1e-6, momentum=0.9, plateau_length=5,
                         plateau_drop=2.0)]
    assert g[1] == len(results) > 0
    _res, seen = _main(["--attack", "pgd", "-archi", "iv", "--wb-ivector", "--bpda", "--input-transform", "ms:7"])
    assert seen[0]["bpda"] is True and "eot_size" not in seen[0]


@pytest.mark.parametrize("extra", [["--attack", "pgd", "-archi", "iv"],                                  # without the switch: as before
                                   ["--attack", "nes", "--wb-ivector"], ["--wb-ivector"],                # the switch belongs to pgd
                                   ["--attack", "pso", "--wb-ivector"],
                                   ["--attack", "pgd", "-archi", "iv", "--wb-ivector", "--eot-size", "2"],
                                   ["--attack", "pgd", "-archi", "iv", "--wb-ivector", "--bpda", "--eot-size", "2"],
                                   ["--attack", "pgd", "-archi", "iv", "--wb-ivector", "--codec", "ulaw"],     # a defence without --bpda
                                   ["--attack", "pgd", "-archi", "iv", "--wb-ivector", "--bpda", "--dither", "1.0"],
                                   ["--attack", "pgd", "-archi", "iv", "--wb-ivector", "--companions", "1"]])
def test_attack_main_refuses_before_any_model_is_built(site, extra):
    built = []
    with pytest.raises(SystemExit):
        _main(extra, built)
    assert built == []
